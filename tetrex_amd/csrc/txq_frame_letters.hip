// Where the letters of every frame window lie and how many stops they hold, on gfx950 (txq_frame_window_letters /
// txq_frame_window_letters_device; `tetrex search --translate --frame-window --verify-frame-windows`).  The
// reference has no counterpart.
//
// The step between translation and count of the verified local search: txq_translate_windows_device has left the windows'
// value ranges, txq_translate_frames_device the frames' residue letters; this call says for window j which letters of the
// frames buffer are its own — the (begin, length) txq_edit_windows_device takes — counts the '*' among them and turns
// (stop-free k-mers, stops) into the threshold txq_count_windows_device takes (fw::stop_threshold).  All the arithmetic is
// txq_frame_windows_plan.hpp's, which tests/native/frame_window_letters_sim.cpp walks on the CPU.
//
// Mapping to the machine: a lane per window, a grid-stride loop over a capped grid.  A lane finds its frame by binary search in
// the window offsets (6 n + 1 words, L2-resident, the probes of neighbouring lanes coincide), its residue range in closed form
// (frame_plan, window_at) and reads its letters as the 16-byte blocks that hold them: one 16-byte load a block, the
// head and the tail of the window masked out, a byte compare and a popcount per 4-byte word.  Neighbouring windows overlap
// W / S-fold in the same bytes; the repeats come from L2 (a batch's frames are a few MiB at the most, and the windows of a
// wave lie within 64 S + W bytes of each other).  The alternative, a wave per frame with a prefix count of stops and the
// windows taking differences, reads every byte once but needs a frame long enough to fill a wave: the frames of short reads
// have a few hundred residues and fewer than ten windows each, so most of its lanes would idle, and a frame of 3 x 10^5
// residues would be one wave's serial walk.  The lane-per-window form keeps every lane busy on both shapes, has no LDS, no
// barrier and no cross-lane traffic, and its redundant loads are hits.
#include "../../include/txq.h"
#include "txq_internal.hpp"
#include "txq_frame_windows_plan.hpp"

namespace txq {
namespace {

constexpr uint32_t kLetterThreads = 256, kLetterBlocks = 1024;

struct LetArgs {
    const uint64_t* rec;  // n + 1
    uint64_t m;           // 6 n frames
    uint32_t k, window, step, edits;
    const uint8_t* frames;
    uint64_t frames_bytes;
    const uint64_t* frame_offsets;  // m + 1
    const uint64_t* win_offsets;    // m + 1
    const uint32_t* win_len;        // n_windows: the windows' stop-free k-mers
    uint64_t n_windows;
    uint64_t* let_begin;
    uint32_t *let_len, *stops, *thresholds;
};

struct GlobalLoad {
    __device__ __forceinline__ text4 operator()(uintptr_t blk, uintptr_t lo, uintptr_t hi) const { return load_block(blk, lo, hi, 0).w; }
};

__global__ __launch_bounds__(kLetterThreads) void frame_window_letters_kernel(LetArgs a) {
    const uintptr_t lo = (uintptr_t)a.frames, hi = lo + a.frames_bytes;
    for (uint64_t j = (uint64_t)blockIdx.x * kLetterThreads + threadIdx.x; j < a.n_windows; j += (uint64_t)kLetterBlocks * kLetterThreads) {
        const fw::Letters at = fw::window_letters(a.rec, a.frame_offsets, a.win_offsets, a.m, j, a.k, a.window, a.step);
        uint32_t s = 0, t = fw::kNotSearched;
        if (fw::letters_inside(at, a.frames_bytes)) {  // (else its pair would be refused by txq_edit_windows_device anyway)
            s = fw::count_stops(lo, hi, lo + at.begin, lo + at.begin + at.len, GlobalLoad{});
            t = fw::stop_threshold(a.win_len[j], s, a.k, a.edits);
        }
        a.let_begin[j] = at.begin;
        a.let_len[j] = at.len;
        a.stops[j] = s;
        a.thresholds[j] = t;
    }
}

int letters_args(size_t n_records, unsigned k, uint32_t window, uint32_t step, const void* rec, const void* frames, size_t frames_bytes,
                 const void* frame_offsets, const void* win_offsets, const void* win_len, size_t n_windows, const void* let_begin, const void* let_len,
                 const void* stops, const void* thresholds) {
    if (k < 1 || k > 12) return fail(TXQ_ERR_ARG, "k = %u: translated k-mers need k in 1..12", k);
    if (window < k || step < 1 || step > window) return fail(TXQ_ERR_ARG, "window = %u, step = %u: windows need window >= k and step in 1..window", window, step);
    if (!frame_offsets || !win_offsets || (n_records && !rec) || (frames_bytes && !frames)) return fail(TXQ_ERR_ARG, "null argument");
    if (n_windows && (!win_len || !let_begin || !let_len || !stops || !thresholds)) return fail(TXQ_ERR_ARG, "null argument");
    if (n_records > 0x7FFFFFFFull / 6) return fail(TXQ_ERR_ARG, "at most 2^31 / 6 records per call");
    if (n_windows > 0xFFFFFFFEull) return fail(TXQ_ERR_ARG, "%zu windows: at most 2^32 - 2 per call", n_windows);
    return TXQ_OK;
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_frame_window_letters_device(const uint64_t* d_rec_offsets, size_t n_records, unsigned k, uint32_t window, uint32_t step, const uint8_t* d_frames,
                                    size_t frames_bytes, const uint64_t* d_frame_offsets, const uint64_t* d_win_offsets, const uint32_t* d_win_len,
                                    size_t n_windows, uint32_t edits, uint64_t* d_let_begin, uint32_t* d_let_len, uint32_t* d_stops, uint32_t* d_thresholds,
                                    void* stream) {
    if (int rc = letters_args(n_records, k, window, step, d_rec_offsets, d_frames, frames_bytes, d_frame_offsets, d_win_offsets, d_win_len, n_windows,
                              d_let_begin, d_let_len, d_stops, d_thresholds))
        return rc;
    if (int rc = require_init()) return rc;
    if (n_windows == 0) return TXQ_OK;
    const LetArgs a{d_rec_offsets, (uint64_t)(6 * n_records), k, window, step, edits, d_frames, (uint64_t)frames_bytes, d_frame_offsets, d_win_offsets,
                    d_win_len, (uint64_t)n_windows, d_let_begin, d_let_len, d_stops, d_thresholds};
    const uint64_t blocks = ((uint64_t)n_windows + kLetterThreads - 1) / kLetterThreads;
    frame_window_letters_kernel<<<(unsigned)(blocks < kLetterBlocks ? blocks : kLetterBlocks), kLetterThreads, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "frame window letters kernel launch");
    return TXQ_OK;
}

int txq_frame_window_letters(const uint64_t* rec_offsets, size_t n_records, unsigned k, uint32_t window, uint32_t step, const uint8_t* frames,
                             size_t frames_bytes, const uint64_t* frame_offsets, const uint64_t* win_offsets, const uint32_t* win_len, size_t n_windows,
                             uint32_t edits, uint64_t* let_begin, uint32_t* let_len, uint32_t* stops, uint32_t* thresholds) {
    if (int rc = letters_args(n_records, k, window, step, rec_offsets, frames, frames_bytes, frame_offsets, win_offsets, win_len, n_windows, let_begin,
                              let_len, stops, thresholds))
        return rc;
    if (int rc = check_ascending(rec_offsets, n_records, "record")) return rc;
    const size_t m = 6 * n_records;
    if (int rc = check_ascending(frame_offsets, m, "frame")) return rc;
    if (int rc = check_ascending(win_offsets, m, "window")) return rc;
    if (frame_offsets[0] != 0 || win_offsets[0] != 0) return fail(TXQ_ERR_ARG, "frame and window offsets begin at 0");
    if (win_offsets[m] > n_windows) return fail(TXQ_ERR_ARG, "the window offsets name more windows than n_windows = %zu", n_windows);
    if (int rc = require_init()) return rc;
    if (n_windows == 0) return TXQ_OK;
    DeviceStage d;  // (+8: no slice of no bytes)
    const size_t s_rec = d.add((n_records + 1) * 8), s_frm = d.add(frames_bytes + 8), s_foff = d.add((m + 1) * 8), s_woff = d.add((m + 1) * 8),
                 s_wlen = d.add(n_windows * 4), s_beg = d.add(n_windows * 8), s_len = d.add(n_windows * 4), s_stop = d.add(n_windows * 4),
                 s_thr = d.add(n_windows * 4);
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> ro = n_records ? rebased(rec_offsets, n_records) : std::vector<uint64_t>{0};
    d.upload(s_rec, ro.data(), ro.size() * 8);
    d.upload(s_frm, frames, frames_bytes);
    d.upload(s_foff, frame_offsets, (m + 1) * 8);
    d.upload(s_woff, win_offsets, (m + 1) * 8);
    d.upload(s_wlen, win_len, n_windows * 4);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_frame_window_letters_device(d.at<uint64_t>(s_rec), n_records, k, window, step, d.at<uint8_t>(s_frm), frames_bytes, d.at<uint64_t>(s_foff),
                                             d.at<uint64_t>(s_woff), d.at<uint32_t>(s_wlen), n_windows, edits, d.at<uint64_t>(s_beg), d.at<uint32_t>(s_len),
                                             d.at<uint32_t>(s_stop), d.at<uint32_t>(s_thr), nullptr);
    if (rc == TXQ_OK) {
        d.download(let_begin, s_beg, n_windows * 8);  // (waits for the kernel)
        d.download(let_len, s_len, n_windows * 4);
        d.download(stops, s_stop, n_windows * 4);
        d.download(thresholds, s_thr, n_windows * 4);
    }
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_frame_window_letters copies");
    return rc;
}

}  // extern "C"
