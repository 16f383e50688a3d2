// Every record of a bin that a WINDOW matches within its cap, for pairs of any number of bins in one call, on gfx950
// (txq_edit_window_targets / txq_edit_window_targets_device; `tetrex search --window --verify-windows --window-targets` and its
// frame-window sibling).  The reference has no counterpart.  The semantics are in include/txq.h: those of
// txq_edit_targets with the window written out as the pattern and the view's records as the one group of a text of its own.
//
// The pipeline is that of txq_edit_targets.hip, kernel by kernel — plan (units and slots per pair), two scans, first keys, the
// walk for W = 1, 2, 4, 8 words, count / scan / write —, and so are the slot arithmetic, the flush rule and the rows
// (txq_edit_targets_plan.hpp).  What differs is how a pair finds its two sides (txq_edit_window_targets_plan.hpp):
//   * the pattern is a window (begin, length) into ONE letter buffer, as in txq_edit_windows.hip: Peq is built from d_letters;
//   * the text is a view of a table, as in txq_edit_align.hip's window form: one entry per resident bin, wherever its records
//     lie.  A unit's pair is uniform over the wave, so its table entry is loaded once per unit into scalar registers;
//   * the bounds that load_block clips its 16-byte loads against are the view's, per unit, not the call's.
// wt_walk_kernel<W> is targets_kernel<W>: one lane per chunk, `best` the least key of the lane's current record, one 64-bit
// atomicMin into the record's slot where the lane leaves a record and once behind its last byte.  No wave reduction — the lanes
// are in different records.  Every pair walks alone (K = 1).
// Everything lives in the caller's workspace; the call allocates nothing, reads nothing back and waits for nothing.
#include <cstddef>

#include "txq_edit_window_targets_plan.hpp"
#include "txq_scan.hpp"

namespace txq {
namespace {

static_assert(wt::kMaxWindow == TXQ_EDIT_MAX_PATTERN, "include/txq.h and the plan header agree");
static_assert(sizeof(wt::View) == sizeof(txq_text_view) && offsetof(wt::View, text) == offsetof(txq_text_view, d_text) &&
                  offsetof(wt::View, rec) == offsetof(txq_text_view, d_rec_offsets) && offsetof(wt::View, n_rec) == offsetof(txq_text_view, n_records) &&
                  offsetof(wt::View, text_bytes) == offsetof(txq_text_view, text_bytes),
              "include/txq.h and the plan header agree on a view");
constexpr uint32_t kDefaultChunk = 512, kMinChunk = 16, kMaxChunk = 1u << 20;  // (those of the search kernels)
constexpr uint32_t kGridBlocks = 256 * 16;  // waves of the persistent grid: 16 per CU

struct WtArgs {
    const uint8_t* letters;
    uint64_t letters_bytes;
    const uint64_t* win_begin;
    const uint32_t* win_len;
    uint64_t n_win;
    const wt::View* views;
    uint64_t n_views;
    const uint32_t* pairs;
    uint64_t n_pairs;
    const uint8_t* codes;
    uint64_t* pref;   // n_pairs + 1: pref[0] = 0, pref[i + 1] = units of pairs 0 .. i
    uint64_t* spref;  // n_pairs + 1: spref[0] = 0, spref[i + 1] = slots of pairs 0 .. i
    uint64_t* slots;  // n_slots keys
    uint64_t* bpref;  // blocks + 1: bpref[0] = 0, bpref[b + 1] = keys in blocks 0 .. b of the slots
    uint64_t n_slots;
    uint32_t* status;
    uint32_t* hits;
    uint64_t capacity;
    uint64_t* total;
    uint32_t chunk;  // bytes of text per lane
};

__device__ __forceinline__ wt::Pair view_pair(const WtArgs& g, uint64_t i) {
    return wt::view_pair(g.pairs, i, g.win_begin, g.win_len, g.n_win, g.letters_bytes, g.views, g.n_views);
}

__global__ __launch_bounds__(256) void wt_plan_kernel(WtArgs g) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) g.pref[0] = 0, g.spref[0] = 0;
    if (i >= g.n_pairs) return;
    const wt::Pair v = view_pair(g, i);
    g.pref[i + 1] = wt::units_of_pair(v, g.chunk);
    g.spref[i + 1] = targets_slots_of(v.ok, 0, v.r1);
    g.status[i] = v.ok ? 0u : kTargetsRefused;
}

// thread i < n_pairs: pair i refused where its slots do not fit; thread s < slots in use: the slot's first key
__global__ __launch_bounds__(256) void wt_init_kernel(WtArgs g) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < g.n_pairs && !targets_fits(g.spref, i, g.n_slots)) g.status[i] = kTargetsRefused;
    if (i >= targets_used(g.spref, g.n_pairs, g.n_slots)) return;
    const uint64_t pair = pair_of_unit(g.spref, g.n_pairs, i);
    uint64_t key = kNoKey;
    if (targets_fits(g.spref, pair, g.n_slots)) {
        const wt::Pair v = view_pair(g, pair);  // (ok: a pair that is not has no slots)
        key = targets_initial_key(v.m, v.e, v.v.rec, i - g.spref[pair], 0, v.gs);
    }
    g.slots[i] = key;
}

__device__ __forceinline__ void lower_slot(uint64_t* slots, uint64_t slot, uint64_t key) {
    if (slot != kNoSlot) atomicMin((unsigned long long*)(slots + slot), (unsigned long long)key);
}

template <int W>
__global__ __launch_bounds__(64) void wt_walk_kernel(WtArgs g) {
    __shared__ uint64_t peq[32 * W];
    __shared__ uint8_t codes[256];
    const uint32_t lane = threadIdx.x;
    const uint64_t total = g.pref[g.n_pairs];
    if (blockIdx.x >= total) return;
    for (uint32_t i = lane; i < 256; i += 64) {
        const uint8_t c = g.codes[i];
        codes[i] = c < 31 ? c : (uint8_t)31;
    }
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t pair = pair_of_unit(g.pref, g.n_pairs, u);
        const wt::Pair v = view_pair(g, pair);  // (uniform over the wave: the table entry stays in scalar registers)
        if (!v.ok || wt::words_of(v.m) != (uint32_t)W || !targets_fits(g.spref, pair, g.n_slots)) continue;
        const uint64_t slice = u - g.pref[pair], base = g.spref[pair];
        const uint64_t* const rec = v.v.rec;
        const uintptr_t text_lo = (uintptr_t)v.v.text, text_hi = text_lo + v.v.text_bytes;  // this unit's view
        __syncthreads();  // the unit before is done with peq
        for (uint32_t i = lane; i < 32 * W; i += 64) peq[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < v.m; i += 64) {
            const uint32_t c = codes[g.letters[v.p0 + i]];
            if (c < 31) atomicOr(reinterpret_cast<uint32_t*>(peq) + 2 * (c * W + (i >> 6)) + ((i >> 5) & 1), 1u << (i & 31));
        }
        __syncthreads();

        const uint32_t m = v.m, e = v.e;
        const uint32_t hw = (m - 1) >> 6, hs = (m - 1) & 63;
        const auto [ca, cb] = chunk_bounds(v.gs, v.ge, slice, 64, lane, g.chunk);
        if (ca < v.ge) {
            uint64_t best = kNoKey;  // of record r
            uint64_t r = record_of(rec, 0, v.r1, ca);
            uint64_t re = rec[r + 1];
            // (offsets that do not ascend cannot take a load outside [gs, ge): every byte index below stays in [start, cb))
            const uint64_t start = wt::walk_start(ca, rec[r], v.gs, wt::lead_of(m, e));
            uint64_t pv[W], mv[W];
#pragma unroll
            for (int w = 0; w < W; ++w) pv[w] = ~0ULL, mv[w] = 0;
            uint32_t score = m;
            const uintptr_t first = (text_lo + start) & ~(uintptr_t)15, last = text_lo + cb;
            for (uintptr_t blk = first; blk < last; blk += 16) {
                const TextBlock raw = load_block(blk, text_lo, text_hi, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t word = raw.w[q];
#pragma nounroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        const uint64_t t = raw.t0 + 4u * q + b;  // (bytes below text_lo: an index >= cb, see load_block)
                        if (t < start || t >= cb) continue;
                        if (t >= re) {  // the record ended: its key goes to its slot, a fresh state in the next one that has bytes
                            lower_slot(g.slots, targets_flush(best, base, r, 0, v.r1), best);
                            best = kNoKey;
                            do {
                                ++r;
                                re = r + 1 <= v.r1 ? rec[r + 1] : v.ge;
                            } while (t >= re && r + 1 < v.r1);
                            if (re > v.ge || t >= re) re = v.ge;
#pragma unroll
                            for (int w = 0; w < W; ++w) pv[w] = ~0ULL, mv[w] = 0;
                            score = m;
                        }
                        const uint32_t cls = codes[(word >> (8 * b)) & 255u];
                        uint64_t carry = 0, ph_in = 0, mh_in = 0;
                        uint32_t hp = 0, hm = 0;
#pragma unroll
                        for (int w = 0; w < W; ++w) {
                            const uint64_t eq = peq[cls * W + w], p = pv[w], n = mv[w];
                            const uint64_t xv = eq | n, x = eq & p;
                            const uint64_t s1 = x + p, s2 = s1 + carry;
                            carry = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
                            const uint64_t xh = (s2 ^ p) | eq;
                            uint64_t ph = n | ~(xh | p), mh = p & xh;
                            if (W == 1 || w >= W / 2) {
                                hp = (uint32_t)w == hw ? (uint32_t)(ph >> hs) & 1u : hp;
                                hm = (uint32_t)w == hw ? (uint32_t)(mh >> hs) & 1u : hm;
                            }
                            const uint64_t ph_out = ph >> 63, mh_out = mh >> 63;
                            ph = (ph << 1) | ph_in;
                            mh = (mh << 1) | mh_in;
                            ph_in = ph_out, mh_in = mh_out;
                            pv[w] = mh | ~(xv | ph);
                            mv[w] = ph & xv;
                        }
                        score += hp - hm;
                        if (t >= ca && score <= e) {
                            const uint64_t key = edit_key(score, t, v.gs, r, 0);
                            best = key < best ? key : best;
                        }
                    }
                }
            }
            lower_slot(g.slots, targets_flush(best, base, r, 0, v.r1), best);  // behind the lane's last byte
        }
    }
}

// keys in block b of the slots -> bpref[b + 1]
__global__ __launch_bounds__(kTargetsBlock) void wt_count_kernel(WtArgs g) {
    __shared__ uint32_t wave_count[kTargetsBlock / 64];
    const uint64_t s = (uint64_t)blockIdx.x * kTargetsBlock + threadIdx.x;
    const bool hit = s < targets_used(g.spref, g.n_pairs, g.n_slots) && g.slots[s] != kNoKey;
    const uint32_t n = (uint32_t)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) g.bpref[0] = 0;
        g.bpref[blockIdx.x + 1] = (uint64_t)wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
    }
}

// blocks 0 .. B - 1: the rows of their slots' keys; block B: the total
__global__ __launch_bounds__(kTargetsBlock) void wt_write_kernel(WtArgs g, uint64_t n_blocks) {
    __shared__ uint32_t wave_count[kTargetsBlock / 64];
    if (blockIdx.x == n_blocks) {
        if (threadIdx.x == 0) *g.total = n_blocks ? g.bpref[n_blocks] : 0;
        return;
    }
    const uint64_t s = (uint64_t)blockIdx.x * kTargetsBlock + threadIdx.x;
    const uint64_t key = s < targets_used(g.spref, g.n_pairs, g.n_slots) ? g.slots[s] : kNoKey;
    const bool hit = key != kNoKey;
    const uint64_t mask = __ballot(hit);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!hit) return;
    uint64_t row = g.bpref[blockIdx.x] + (uint64_t)__popcll(mask & ((1ULL << lane) - 1));
    for (uint32_t k = 0; k < wave; ++k) row += wave_count[k];
    if (row >= g.capacity) return;
    const uint64_t pair = pair_of_unit(g.spref, g.n_pairs, s);
    const wt::Pair v = view_pair(g, pair);
    targets_row(g.hits + 4 * row, pair, key, v.v.rec, 0, v.r1, v.gs);
}

// what both entry points can see of their arguments
int wt_args(const void* letters, size_t letters_bytes, const void* win_begin, const void* win_len, size_t n_windows, const void* views, size_t n_views,
            const void* pairs, size_t n_pairs, const void* codes, const void* hits, size_t capacity, const void* total, const void* status, size_t n_slots) {
    if (!codes || !total || (n_pairs && (!pairs || !status)) || (capacity && !hits) || (n_windows && (!win_begin || !win_len)) || (n_views && !views) ||
        (letters_bytes && !letters))
        return fail(TXQ_ERR_ARG, "null argument");
    if (n_pairs > 0x7FFFFFFFull) return fail(TXQ_ERR_ARG, "at most 2^31 - 1 pairs per call");
    if (n_slots >= 1ULL << 38 || capacity >= 1ULL << 38) return fail(TXQ_ERR_ARG, "at most 2^38 slots and rows per call");
    return TXQ_OK;
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_edit_window_targets_device(const uint8_t* d_letters, size_t letters_bytes, const uint64_t* d_win_begin, const uint32_t* d_win_len, size_t n_windows,
                                   const txq_text_view* d_views, size_t n_views, const uint32_t* d_pairs, size_t n_pairs, const uint8_t* d_codes,
                                   uint32_t* d_hits, size_t capacity, uint64_t* d_total, uint32_t* d_status, size_t n_slots, void* d_workspace, void* stream) {
    if (int rc = wt_args(d_letters, letters_bytes, d_win_begin, d_win_len, n_windows, d_views, n_views, d_pairs, n_pairs, d_codes, d_hits, capacity, d_total,
                         d_status, n_slots))
        return rc;
    if (n_pairs && (!d_workspace || ((uintptr_t)d_workspace & 7))) return fail(TXQ_ERR_ARG, "the workspace must be an 8-byte aligned device pointer");
    if (int rc = require_init()) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_pairs == 0) n_slots = 0;
    const uint64_t n_blocks = targets_blocks(n_slots);
    const uint32_t chunk = (env_u32("TXQ_EDIT_CHUNK", kDefaultChunk, kMinChunk, kMaxChunk) + 15) / 16 * 16;
    uint64_t* const ws = (uint64_t*)d_workspace;  // unit prefix, slot prefix, slots, block prefix: TXQ_EDIT_WINDOW_TARGETS_WORKSPACE
    const WtArgs g{d_letters, letters_bytes, d_win_begin, d_win_len, n_windows, reinterpret_cast<const wt::View*>(d_views), n_views, d_pairs, n_pairs, d_codes,
                   ws, ws + (n_pairs + 1), ws + 2 * (n_pairs + 1), ws + 2 * (n_pairs + 1) + n_slots, n_slots, d_status, d_hits, capacity, d_total, chunk};
    if (n_pairs) {
        const unsigned per_pair = (unsigned)((n_pairs + 255) / 256);
        const uint64_t most = n_pairs > n_slots ? n_pairs : n_slots;
        wt_plan_kernel<<<per_pair, 256, 0, st>>>(g);
        scan_kernel<<<1, 1024, 0, st>>>(g.pref + 1, n_pairs);
        scan_kernel<<<1, 1024, 0, st>>>(g.spref + 1, n_pairs);
        wt_init_kernel<<<(unsigned)((most + 255) / 256), 256, 0, st>>>(g);
        wt_walk_kernel<1><<<kGridBlocks, 64, 0, st>>>(g);
        wt_walk_kernel<2><<<kGridBlocks, 64, 0, st>>>(g);
        wt_walk_kernel<4><<<kGridBlocks, 64, 0, st>>>(g);
        wt_walk_kernel<8><<<kGridBlocks, 64, 0, st>>>(g);
        if (n_blocks) {
            wt_count_kernel<<<(unsigned)n_blocks, kTargetsBlock, 0, st>>>(g);
            scan_kernel<<<1, 1024, 0, st>>>(g.bpref + 1, n_blocks);
        }
    }
    wt_write_kernel<<<(unsigned)n_blocks + 1, kTargetsBlock, 0, st>>>(g, n_blocks);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "edit window targets kernel launch");
    return TXQ_OK;
}

int txq_edit_window_targets(const uint8_t* letters, size_t letters_bytes, const uint64_t* win_begin, const uint32_t* win_len, size_t n_windows,
                            const txq_text_view* views, size_t n_views, const uint32_t* pairs, size_t n_pairs, const uint8_t* codes, uint32_t* hits,
                            size_t capacity, uint64_t* total, uint32_t* status, size_t n_slots) {
    if (int rc = wt_args(letters, letters_bytes, win_begin, win_len, n_windows, views, n_views, pairs, n_pairs, codes, hits, capacity, total, status, n_slots))
        return rc;
    // every text at a 16-byte boundary of one slice, every view's offsets behind those of the view before
    std::vector<uint64_t> text_at(n_views), rec_at(n_views);
    uint64_t texts_bytes = 0, n_offsets = 0;
    for (size_t g = 0; g < n_views; ++g) {
        const txq_text_view& v = views[g];
        if (!v.d_rec_offsets || (v.text_bytes && !v.d_text)) return fail(TXQ_ERR_ARG, "null argument");
        if (v.n_records >= 0xFFFFFFFEull) return fail(TXQ_ERR_ARG, "at most 2^32 - 2 records per view");
        if (v.text_bytes + v.n_records >= 1ULL << kPosBits) return fail(TXQ_ERR_ARG, "text too large for one call");
        if (int rc = check_ascending(v.d_rec_offsets, v.n_records, "record", "text", v.text_bytes)) return rc;
        if (v.d_rec_offsets[0] > v.text_bytes) return fail(TXQ_ERR_ARG, "record offsets are not ascending within the text at record 0");
        text_at[g] = texts_bytes, rec_at[g] = n_offsets;
        texts_bytes += (v.text_bytes + 15) & ~(uint64_t)15;
        n_offsets += v.n_records + 1;
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
        if (p >= n_windows || g >= n_views) return fail(TXQ_ERR_ARG, "pair %zu names window %u of %zu, view %u of %zu", i, p, n_windows, g, n_views);
        const uint64_t m = win_len[p], b = win_begin[p];
        if (m < 1 || m > wt::kMaxWindow) return fail(TXQ_ERR_ARG, "pair %zu: a window of %llu bytes (1..%u run on the device)", i, (unsigned long long)m, wt::kMaxWindow);
        if (b > letters_bytes || m > letters_bytes - b) return fail(TXQ_ERR_ARG, "pair %zu: window %u leaves the %zu letters", i, p, letters_bytes);
    }
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) n_slots = 0;
    DeviceStage d;  // (+16: the kernel's 16-byte loads of text end inside the slice)
    const size_t s_let = d.add(letters_bytes + 16), s_wb = d.add(n_windows * 8 + 8), s_wl = d.add(n_windows * 4 + 4), s_text = d.add(texts_bytes + 16),
                 s_rec = d.add(n_offsets * 8 + 8), s_views = d.add(n_views * sizeof(txq_text_view) + 8), s_pairs = d.add(n_pairs * 12 + 4), s_codes = d.add(256),
                 s_hits = d.add(capacity * 16 + 4), s_total = d.add(8), s_status = d.add(n_pairs * 4 + 4),
                 s_work = d.add(TXQ_EDIT_WINDOW_TARGETS_WORKSPACE(n_pairs, n_slots));
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    std::vector<txq_text_view> table(n_views);
    for (size_t g = 0; g < n_views; ++g) {
        const txq_text_view& v = views[g];
        d.upload(s_text + text_at[g], v.d_text, v.text_bytes);
        d.upload(s_rec + 8 * rec_at[g], v.d_rec_offsets, (v.n_records + 1) * 8);
        table[g] = {d.at<uint8_t>(s_text) + text_at[g], d.at<uint64_t>(s_rec) + rec_at[g], v.n_records, v.text_bytes};
    }
    d.upload(s_let, letters, letters_bytes);
    d.upload(s_wb, win_begin, n_windows * 8);
    d.upload(s_wl, win_len, n_windows * 4);
    d.upload(s_views, table.data(), n_views * sizeof(txq_text_view));
    d.upload(s_pairs, pairs, n_pairs * 12);
    d.upload(s_codes, codes, 256);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_edit_window_targets_device(d.at<uint8_t>(s_let), letters_bytes, d.at<uint64_t>(s_wb), d.at<uint32_t>(s_wl), n_windows,
                                            d.at<txq_text_view>(s_views), n_views, d.at<uint32_t>(s_pairs), n_pairs, d.at<uint8_t>(s_codes),
                                            d.at<uint32_t>(s_hits), capacity, d.at<uint64_t>(s_total), d.at<uint32_t>(s_status), n_slots, d.at<void>(s_work), nullptr);
    if (rc == TXQ_OK) {
        d.download(total, s_total, 8);  // (waits for the kernels)
        d.download(status, s_status, n_pairs * 4);
        if (d.error() == hipSuccess) d.download(hits, s_hits, (size_t)(*total < capacity ? *total : capacity) * 16);
    }
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_edit_window_targets copies");
    return rc;
}

}  // extern "C"
