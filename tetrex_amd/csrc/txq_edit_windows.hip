// Approximate matching of (window, bin) pairs by edit distance on gfx950 (txq_edit_windows / txq_edit_windows_device;
// `tetrex search --window --verify-windows`).  The reference has no counterpart.  The semantics are in
// include/txq.h: those of txq_edit_search with window p written out as pattern p.
//
// The patterns are windows into ONE letter buffer (they overlap W/S-fold and are never written out), and the windows of a
// record that hit one bin come as a run of consecutive pairs of one group.  edit_windows_kernel<W, K> is edit_kernel of
// txq_edit.hip — Myers' recurrence with the pattern one integer of W words, units of 64 lane chunks, a persistent grid, one
// 64-bit key per pair — with K independent states per lane: a lane loads each 16-byte block of its chunk once, extracts each
// byte, looks up its class and handles a record's end once, and then steps the K states of its bundle.  Each state has its own
// Pv / Mv in VGPRs, its own m, score bit and cap, its own Peq rows in LDS (K W <= 8 words a class: 2 KiB as before) and its own
// running best key; per state there is a wave minimum and one atomicMin on that pair's key.
//
// Bundles are cut by edit_windows_plan_kernel with the rules of txq_edit_windows_plan.hpp (a head every K pairs, at a change
// of group or word count and at a refused pair); heads carry the units of their group's text, so scan_kernel and pair_of_unit
// hand out (bundle, slice) as they hand out (pair, slice) elsewhere.  The walk starts at the largest lead-in of the bundle.
// Nine instances — (W, K) with K W <= 8, K = 1, 2, 4 — of which a call launches four, one per word count, with K the bundle
// size of that word count under the call's cap: a unit is walked by the instance of its word count, a bundle of fewer than K
// pairs with the other states idle, and skipped by the others.  As many launches as txq_edit_search_device makes.
// How many pairs walk together is a matter of load ("Measured"): a wave that steps K states takes K times as
// long over its chunk, which pays only where there are more waves than the machine holds at once.  Unless
// TXQ_EDIT_WINDOWS_BUNDLE says otherwise, a call of fewer than kFillPairs pairs therefore walks every pair alone.
#include "txq_edit_common.hpp"
#include "txq_edit_windows_plan.hpp"
#include "txq_scan.hpp"

namespace txq {
namespace {

constexpr uint32_t kMaxWindow = TXQ_EDIT_MAX_PATTERN;
constexpr uint32_t kDefaultChunk = 512, kMinChunk = 16, kMaxChunk = 1u << 20;
constexpr uint32_t kDefaultBundle = 4;     // the fastest measured on a full machine
constexpr uint32_t kFillPairs = 8192;     // 256 CUs x 4 SIMDs x 8 waves: below it every pair has a wave slot of its own
constexpr uint32_t kGridBlocks = 256 * 16;  // waves of the persistent grid: 16 per CU

struct EwArgs {
    const uint8_t* letters;
    uint64_t letters_bytes;
    const uint64_t* win_begin;
    const uint32_t* win_len;
    uint64_t n_win;
    TextGroups t;
    const uint32_t* pairs;
    uint64_t n_pairs;
    const uint8_t* codes;
    uint32_t* out;
    uint64_t* keys;  // n_pairs
    uint64_t* pref;  // n_pairs + 1: pref[0] = 0, pref[i + 1] = units of pairs 0 .. i (heads only)
    uint32_t chunk;  // bytes of text per lane
    uint32_t cap;    // pairs of a bundle at most (TXQ_EDIT_WINDOWS_BUNDLE)
};

// What a pair works on; ok = false: an index outside its array, a window of no letters, of more than kMaxWindow or one that
// leaves the letter buffer, a group whose offsets leave theirs.
struct WinView {
    bool ok;
    uint32_t m, e, g;
    uint64_t p0, r0, r1, gs, ge;
};

__device__ __forceinline__ WinView view_window(const EwArgs& a, uint64_t i) {
    WinView v{};
    const uint32_t p = a.pairs[3 * i];
    v.g = a.pairs[3 * i + 1];
    v.e = a.pairs[3 * i + 2];
    if (p >= a.n_win) return v;
    const uint64_t p0 = a.win_begin[p];
    const uint32_t m = a.win_len[p];
    if (m == 0 || m > kMaxWindow || p0 > a.letters_bytes || m > a.letters_bytes - p0) return v;
    const GroupView gv = view_group(a.t, v.g);
    v.ok = gv.ok;
    v.m = m;
    v.p0 = p0, v.r0 = gv.r0, v.r1 = gv.r1, v.gs = gv.gs, v.ge = gv.ge;
    return v;
}

__device__ __forceinline__ ew::Member member_of(const WinView& v) { return {v.ok, v.g, v.ok ? ew::words_of(v.m) : 0u}; }

__global__ __launch_bounds__(256) void edit_windows_plan_kernel(EwArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) a.pref[0] = 0;
    if (i >= a.n_pairs) return;
    const WinView v = view_window(a, i);
    uint64_t units = 0, key = kBadPair;
    if (v.ok) {
        const ew::Member prev = i ? member_of(view_window(a, i - 1)) : ew::Member{};
        if (ew::is_head(i, prev, member_of(v), a.cap)) units = units_of(v.ge - v.gs, 64, a.chunk);
        // end 0 of the group's first record: distance m, the lowest position there is
        key = v.r1 > v.r0 && v.m <= v.e ? (uint64_t)v.m << kPosBits : kNoKey;
    }
    a.pref[i + 1] = units;
    a.keys[i] = key;
}

template <int W, int K>
__global__ __launch_bounds__(64) void edit_windows_kernel(EwArgs a) {
    static_assert(K * W <= 8 && K <= (int)ew::kMaxBundle, "the states of a bundle stay in registers");
    __shared__ uint64_t peq[K * 32 * W];
    __shared__ uint8_t codes[256];
    const uint32_t lane = threadIdx.x;
    const uint64_t total = a.pref[a.n_pairs];
    if (blockIdx.x >= total) return;
    for (uint32_t i = lane; i < 256; i += 64) {
        const uint8_t c = a.codes[i];
        codes[i] = c < 31 ? c : (uint8_t)31;
    }
    const uintptr_t text_lo = (uintptr_t)a.t.text, text_hi = text_lo + a.t.text_bytes;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t head = pair_of_unit(a.pref, a.n_pairs, u);
        const WinView v = view_window(a, head);
        if (!v.ok || ew::words_of(v.m) != (uint32_t)W) continue;  // (uniform over the wave)
        const uint32_t n = ew::bundle_extent(head, a.n_pairs, a.cap, [&](uint64_t i) { return member_of(view_window(a, i)); });
        const uint64_t slice = u - a.pref[head];
        // the states: state k is pair head + k (k < n; the others stay idle)
        uint32_t m[K], e[K], hw[K], hs[K];
        uint64_t p0[K], lead = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const WinView vk = k == 0 || (uint32_t)k >= n ? v : view_window(a, head + k);
            m[k] = vk.m, e[k] = vk.e, p0[k] = vk.p0;
            hw[k] = (vk.m - 1) >> 6, hs[k] = (vk.m - 1) & 63;
            const uint64_t l = ew::lead_of(vk.m, vk.e);
            lead = l > lead ? l : lead;
        }
        __syncthreads();  // the unit before is done with peq
        for (uint32_t i = lane; i < K * 32 * W; i += 64) peq[i] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((uint32_t)k >= n) continue;
            for (uint32_t i = lane; i < m[k]; i += 64) {
                const uint32_t c = codes[a.letters[p0[k] + i]];
                if (c < 31) atomicOr(reinterpret_cast<uint32_t*>(peq) + 2 * ((k * 32 + c) * W + (i >> 6)) + ((i >> 5) & 1), 1u << (i & 31));
            }
        }
        __syncthreads();

        const auto [ca, cb] = chunk_bounds(v.gs, v.ge, slice, 64, lane, a.chunk);
        uint64_t best[K];
#pragma unroll
        for (int k = 0; k < K; ++k) best[k] = kNoKey;
        if (ca < v.ge) {
            uint64_t r = record_of(a.t.rec, v.r0, v.r1, ca);
            uint64_t rs = a.t.rec[r], re = a.t.rec[r + 1];
            // (offsets that do not ascend cannot take a load outside [gs, ge): every byte index below stays in [start, cb))
            if (rs < v.gs || rs > ca) rs = ca;
            const uint64_t start = ew::walk_start(ca, rs, lead);
            uint64_t pv[K][W], mv[K][W];
            uint32_t score[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int w = 0; w < W; ++w) pv[k][w] = ~0ULL, mv[k][w] = 0;
                score[k] = m[k];
            }
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
                        if (t >= re) {  // the record ended: fresh states in the next one that has bytes
                            do {
                                ++r;
                                re = r + 1 <= v.r1 ? a.t.rec[r + 1] : v.ge;
                            } while (t >= re && r + 1 < v.r1);
                            if (re > v.ge || t >= re) re = v.ge;
#pragma unroll
                            for (int k = 0; k < K; ++k) {
#pragma unroll
                                for (int w = 0; w < W; ++w) pv[k][w] = ~0ULL, mv[k][w] = 0;
                                score[k] = m[k];
                            }
                        }
                        const uint32_t cls = codes[(word >> (8 * b)) & 255u];
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            if (k > 0 && (uint32_t)k >= n) continue;  // (uniform over the wave; a bundle has a first pair)
                            uint64_t carry = 0, ph_in = 0, mh_in = 0;
                            uint32_t hp = 0, hm = 0;
#pragma unroll
                            for (int w = 0; w < W; ++w) {
                                const uint64_t eq = peq[(k * 32 + cls) * W + w], p = pv[k][w], nn = mv[k][w];
                                const uint64_t xv = eq | nn, x = eq & p;
                                const uint64_t s1 = x + p, s2 = s1 + carry;
                                carry = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
                                const uint64_t xh = (s2 ^ p) | eq;
                                uint64_t ph = nn | ~(xh | p), mh = p & xh;
                                if (W == 1 || w >= W / 2) {
                                    hp = (uint32_t)w == hw[k] ? (uint32_t)(ph >> hs[k]) & 1u : hp;
                                    hm = (uint32_t)w == hw[k] ? (uint32_t)(mh >> hs[k]) & 1u : hm;
                                }
                                const uint64_t ph_out = ph >> 63, mh_out = mh >> 63;
                                ph = (ph << 1) | ph_in;
                                mh = (mh << 1) | mh_in;
                                ph_in = ph_out, mh_in = mh_out;
                                pv[k][w] = mh | ~(xv | ph);
                                mv[k][w] = ph & xv;
                            }
                            score[k] += hp - hm;
                            if (t >= ca && score[k] <= e[k]) {
                                const uint64_t key = (uint64_t)score[k] << kPosBits | (t - v.gs + 1 + (r - v.r0));
                                best[k] = key < best[k] ? key : best[k];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((uint32_t)k >= n) continue;
            uint64_t least = best[k];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const uint64_t o = __shfl_xor(least, d);
                least = o < least ? o : least;
            }
            if (lane == 0 && least != kNoKey) atomicMin((unsigned long long*)(a.keys + head + k), (unsigned long long)least);
        }
    }
}

// keys into (d, r, j): what edit_finish_kernel of txq_edit_common.hpp does, on a window's view of its pair
__global__ __launch_bounds__(256) void edit_windows_finish_kernel(EwArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_pairs) return;
    const uint64_t key = a.keys[i];
    uint32_t d = 0xFFFFFFFFu, r = 0xFFFFFFFFu, j = 0xFFFFFFFFu;
    if (key == kBadPair) r = j = 0xFFFFFFFEu;
    else if (key != kNoKey) {
        const WinView v = view_window(a, i);
        const EditAnswer ans = edit_answer(key, a.t.rec, v.r0, v.r1, v.gs);
        d = ans.d, r = ans.r, j = ans.j;
    }
    a.out[3 * i] = d;
    a.out[3 * i + 1] = r;
    a.out[3 * i + 2] = j;
}

// the instance of W words that holds the bundles of the call's cap
template <int W>
void launch_walk(const EwArgs& a, hipStream_t st) {
    const uint32_t k = ew::bundle_size(W, a.cap);
    if constexpr (W <= 2) {
        if (k == 4) return (void)edit_windows_kernel<W, 4><<<kGridBlocks, 64, 0, st>>>(a);
    }
    if constexpr (W <= 4) {
        if (k == 2) return (void)edit_windows_kernel<W, 2><<<kGridBlocks, 64, 0, st>>>(a);
    }
    edit_windows_kernel<W, 1><<<kGridBlocks, 64, 0, st>>>(a);
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_edit_windows_device(const uint8_t* d_letters, size_t letters_bytes, const uint64_t* d_win_begin, const uint32_t* d_win_len, size_t n_windows,
                            const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                            const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs, const uint8_t* d_codes,
                            uint32_t* d_out, void* d_workspace, void* stream) {
    if (!d_win_begin || !d_win_len) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = edit_device_args(d_letters, d_win_begin, letters_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, d_pairs, n_pairs,
                                  d_codes, d_out, d_workspace))
        return rc;
    if (n_pairs == 0) return TXQ_OK;
    hipStream_t st = (hipStream_t)stream;
    void* scratch = d_workspace;  // keys and prefix: TXQ_EDIT_WINDOWS_WORKSPACE(n_pairs) bytes of the caller's
    const uint32_t chunk = (env_u32("TXQ_EDIT_CHUNK", kDefaultChunk, kMinChunk, kMaxChunk) + 15) / 16 * 16;
    const uint32_t asked = env_u32("TXQ_EDIT_WINDOWS_BUNDLE", n_pairs < kFillPairs ? 1u : kDefaultBundle, 1, ew::kMaxBundle);
    const uint32_t cap = asked >= 4 ? 4u : asked >= 2 ? 2u : 1u;
    const EwArgs a{d_letters, letters_bytes, d_win_begin, d_win_len, n_windows, {d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, n_groups},
                   d_pairs, n_pairs, d_codes, d_out, (uint64_t*)scratch, (uint64_t*)scratch + n_pairs, chunk, cap};
    const unsigned per_pair = (unsigned)((n_pairs + 255) / 256);
    edit_windows_plan_kernel<<<per_pair, 256, 0, st>>>(a);
    scan_kernel<<<1, 1024, 0, st>>>(a.pref + 1, n_pairs);
    launch_walk<1>(a, st);
    launch_walk<2>(a, st);
    launch_walk<4>(a, st);
    launch_walk<8>(a, st);
    edit_windows_finish_kernel<<<per_pair, 256, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "edit windows kernel launch");
    return TXQ_OK;
}

int txq_edit_windows(const uint8_t* letters, size_t letters_bytes, const uint64_t* win_begin, const uint32_t* win_len, size_t n_windows,
                     const uint8_t* text, const uint64_t* rec_offsets, size_t n_records, const uint64_t* group_offsets, size_t n_groups,
                     const uint32_t* pairs, size_t n_pairs, const uint8_t* codes, uint32_t* out) {
    if (!rec_offsets || !group_offsets || (n_windows && (!win_begin || !win_len))) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = check_ascending(rec_offsets, n_records, "record")) return rc;
    if (int rc = check_ascending(group_offsets, n_groups, "group", "records", n_records)) return rc;
    const uint64_t text0 = rec_offsets[0], text_bytes = rec_offsets[n_records] - text0;
    if (int rc = edit_args(rec_offsets, rec_offsets, group_offsets, pairs, n_pairs, n_records, text_bytes, codes, out)) return rc;
    if ((letters_bytes && !letters) || (text_bytes && !text)) return fail(TXQ_ERR_ARG, "null argument");
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
        if (p >= n_windows || g >= n_groups) return fail(TXQ_ERR_ARG, "pair %zu names window %u of %zu, group %u of %zu", i, p, n_windows, g, n_groups);
        const uint64_t m = win_len[p], b = win_begin[p];
        if (m < 1 || m > kMaxWindow) return fail(TXQ_ERR_ARG, "pair %zu: a window of %llu bytes (1..%u run on the device)", i, (unsigned long long)m, kMaxWindow);
        if (b > letters_bytes || m > letters_bytes - b) return fail(TXQ_ERR_ARG, "pair %zu: window %u leaves the %zu letters", i, p, letters_bytes);
    }
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) return TXQ_OK;
    DeviceStage d;  // (+16: the kernel's 16-byte loads of text end inside the slice)
    const size_t s_let = d.add(letters_bytes + 16), s_wb = d.add(n_windows * 8 + 8), s_wl = d.add(n_windows * 4 + 4), s_text = d.add(text_bytes + 16),
                 s_rec = d.add((n_records + 1) * 8), s_grp = d.add((n_groups + 1) * 8), s_pairs = d.add(n_pairs * 12), s_codes = d.add(256),
                 s_out = d.add(n_pairs * 12), s_work = d.add(TXQ_EDIT_WINDOWS_WORKSPACE(n_pairs));
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> ro = rebased(rec_offsets, n_records);
    d.upload(s_let, letters, letters_bytes);
    d.upload(s_wb, win_begin, n_windows * 8);
    d.upload(s_wl, win_len, n_windows * 4);
    d.upload(s_text, text + text0, text_bytes);
    d.upload(s_rec, ro.data(), ro.size() * 8);
    d.upload(s_grp, group_offsets, (n_groups + 1) * 8);
    d.upload(s_pairs, pairs, n_pairs * 12);
    d.upload(s_codes, codes, 256);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_edit_windows_device(d.at<uint8_t>(s_let), letters_bytes, d.at<uint64_t>(s_wb), d.at<uint32_t>(s_wl), n_windows, d.at<uint8_t>(s_text),
                                     d.at<uint64_t>(s_rec), n_records, text_bytes, d.at<uint64_t>(s_grp), n_groups, d.at<uint32_t>(s_pairs), n_pairs,
                                     d.at<uint8_t>(s_codes), d.at<uint32_t>(s_out), d.at<void>(s_work), nullptr);
    if (rc == TXQ_OK) d.download(out, s_out, n_pairs * 12);  // (waits for the kernels)
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_edit_windows copies");
    return rc;
}

}  // extern "C"
