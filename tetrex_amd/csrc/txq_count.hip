// Threshold membership of value sets on gfx950 (txq_count / txq_count_device): seqan::hibf
// membership_agent::membership_for(values, threshold) on an HIBF, counting_agent::bulk_count plus a threshold on a flat IBF.
// The reference only ever asks for one value at threshold 1 (include/index_hibf.h:142-147); this is the general query.
//
// Query q owns values [offsets[q], offsets[q+1]) and a threshold t_q.  count[q][b] = how many of its values have bit b in
// bulk_contains; hit[q][b] = count[q][b] >= t_q.  On an HIBF the count of a technical bin steers the descent exactly as
// Hibf::descend walks it (oracle/txo_ibf.hpp), with counts in place of one bit: runs of technical bins of one user bin are
// summed, a merged bin is visited when its count reaches t_q, a run whose sum reaches t_q is a hit.
//
// Mapping to the machine:
//   * the row gather is the probe's (txq_probe.hip): LPK lanes x 16-byte loads per value, LPK = pow2 >= the row's 16-byte
//     chunks (<= 64; wider rows are cut into column tiles of 64 chunks), 64 / LPK values per step, two steps in flight;
//   * every set bit of a lane's ANDed 128 bits is one LDS atomic add to the workgroup's u32 counters (chunk c, bin b at
//     c * 129 + b: lanes of different chunks hit different banks; lanes of one chunk in different values may add to the same
//     counter, which the LDS serialises).  Bit-sliced counters in VGPRs were measured and dropped: on
//     300-value queries their flushes cost more than the atomics they save;
//   * at the end of a query the counters are thresholded and written once per (query, word): a hit word by ballot, and the
//     64 u32 counts of the word as one coalesced 256-byte store.  No per-value mask is written; bytes per value h*W*8 + 8.
// Flat IBF: the value array is cut into units of `seg` values (seg_len, txq_count_plan.hpp: the unit arithmetic lives there,
// where tests/native/count_units_sim.cpp runs it on the CPU); a unit starts at a query boundary unless the query
// is longer than `seg`, so a short query is counted by ONE workgroup (four waves that share its LDS counters) and written
// directly, and a long one (10^6 values) is spread over many workgroups that add their partial counts to a per-query row of
// u32 accumulators (one global atomic per non-zero bin and workgroup); count_finish_kernel thresholds those rows and answers
// the empty queries.
// HIBF: level-synchronous work items (query, IBF) as in hibf_level_kernel; one wave counts all values of the query on the
// IBF, walks its technical bins (one lane per bin; a run's last lane sums the run), writes the user bins of this shard's
// columns and appends (query, child) for merged bins that pass.  Each level reads its item count from HBM: no host
// synchronisation inside a call.
#include "txq_internal.hpp"
#include "txq_count_plan.hpp"
#include "txq_count_windows_plan.hpp"
#include "txq_count_windows_tree_plan.hpp"
#include <algorithm>

namespace txq {

typedef uint32_t cx4 __attribute__((ext_vector_type(4)));

static constexpr uint32_t kLdsPitch = 129;      // u32 counters of chunk c at lds[c * 129 + b], b < 128
static constexpr uint32_t kTileChunks = 64;     // 16-byte chunks per column tile (8192 bins)
static constexpr int kFlatWaves = 4;            // waves of a flat workgroup: they share one unit and its LDS counters
static constexpr uint32_t kWindowsWaves = 1;    // waves of a sliding-window workgroup: 1 or 4 (TXQ_COUNT_WINDOWS_WAVES; DESIGN.md §17: one wave won)

struct CountOut {
    const uint64_t* values;
    const uint64_t* offsets;  // nq + 1
    const uint32_t* lens;     // null, or nq lengths: query q owns [offsets[q], offsets[q] + lens[q]) (txq_count_windows on an HIBF)
    const uint32_t* thr;      // nq
    uint64_t* hits;           // [nq][W]
    uint32_t* counts;         // [nq][64 W] or null
    uint32_t* acc;            // flat: long queries' accumulators [nq][64 W] (== counts when counts are asked for)
    unsigned long long* trace;  // null, or [kCwTraceSlots][kCwTraceWords] totals of txq_count_windows on an HIBF (txq_count_windows_trace)
    uint64_t user_bins;       // bits of a full mask (t = 0 selects only these)
    uint32_t nq, W, word0;
};

// Count values [lo, hi) on the column tile of chunks [c0, c0 + 2^lpk_log2) of IBF f into the workgroup's LDS counters: wave
// `wave` of `n_waves` takes every n_waves-th pair of steps.  H: hash functions loaded per value (an IBF with fewer repeats its
// last row).  lo, hi are workgroup-uniform.  SUB: the values LEAVE the counters (txq_count_windows): one atomic subtraction per
// set bit, on the same counters.
template <int H, bool SUB = false>
__device__ __forceinline__ void count_values(const IbfDev& f, uint32_t lpk_log2, uint32_t c0, uint32_t chunks, const uint64_t* __restrict__ values,
                                             uint64_t lo, uint64_t hi, uint32_t* lds, uint32_t wave = 0, uint32_t n_waves = 1) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t sub = lane & ((1u << lpk_log2) - 1u), grp = lane >> lpk_log2, kps = 64u >> lpk_log2;
    const uint32_t c = c0 + sub;
    const bool mine = c < chunks;
    const bool w1 = f.stride == 1;  // rows of one word: 8-byte loads
    uint32_t* cnt = lds + sub * kLdsPitch;
    for (uint64_t i0 = lo + (uint64_t)wave * 2u * kps; i0 < hi; i0 += (uint64_t)n_waves * 2u * kps) {
        cx4 x[2][H];
        bool ok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint64_t i = i0 + u * kps + grp;
            ok[u] = i < hi && mine;
            const uint64_t v = i < hi ? values[i] : 0;
            uint64_t row = 0;
#pragma unroll
            for (int j = 0; j < H; ++j) {
                if (j == 0 || (uint32_t)j < f.hash_funs) row = hash_row(v, kSeeds[j], f.hash_shift, f.bin_size);
                const uint64_t* p = f.words + row * f.stride + 2u * c;
                if (!ok[u]) x[u][j] = cx4{0u, 0u, 0u, 0u};
                else if (w1) {
                    const uint64_t w = *p;
                    x[u][j] = cx4{(uint32_t)w, (uint32_t)(w >> 32), 0u, 0u};
                } else x[u][j] = *reinterpret_cast<const cx4*>(p);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            cx4 a = x[u][0];
#pragma unroll
            for (int j = 1; j < H; ++j) a &= x[u][j];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t m = a[d];
                while (m) {
                    if (SUB) atomicSub(cnt + d * 32 + (uint32_t)__builtin_ctz(m), 1u);
                    else atomicAdd(cnt + d * 32 + (uint32_t)__builtin_ctz(m), 1u);
                    m &= m - 1u;
                }
            }
        }
    }
}

// ---- flat IBF -----------------------------------------------------------------------------------------------------------

// Units of `seg` values (grid-stride over units x column tiles), kFlatWaves waves per unit.  Dynamic LDS: min(chunks, 64) * 129 u32.
template <int H>
__global__ __launch_bounds__(64 * kFlatWaves) void count_flat_kernel(IbfDev f, CountOut o, uint32_t lpk_log2, uint32_t n_tiles) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
    const uint32_t tile = 1u << lpk_log2;
    for (uint32_t i = threadIdx.x; i < (chunks < tile ? chunks : tile) * kLdsPitch; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    const uint64_t base = o.offsets[0], end = o.offsets[o.nq];
    if (end <= base) return;
    const uint64_t seg = seg_len(end - base), n_units = (end - base + seg - 1) / seg;
    const size_t W = o.W;
    for (uint64_t work = blockIdx.x; work < n_units * n_tiles; work += gridDim.x) {
        const uint64_t u = work / n_tiles;
        const uint32_t c0 = (uint32_t)(work % n_tiles) << lpk_log2;
        const uint32_t tcn = chunks - c0 < tile ? chunks - c0 : tile;  // chunks of this tile
        const uint64_t lo = unit_start(o.offsets, o.nq, end, seg, base + u * seg);
        const uint64_t hi = u + 1 == n_units ? end : unit_start(o.offsets, o.nq, end, seg, base + (u + 1) * seg);
        if (lo >= hi) continue;
        uint32_t q = query_of(o.offsets, o.nq, lo);
        uint64_t pos = lo;
        while (pos < hi) {
            const uint64_t qb = o.offsets[q], qe = o.offsets[q + 1];
            const uint64_t stop = qe < hi ? qe : hi;
            count_values<H>(f, lpk_log2, c0, chunks, o.values, pos, stop, lds, wave, kFlatWaves);
            __syncthreads();
            const bool whole = qe - qb <= seg;  // (then the whole query lies in this unit)
            const uint32_t t = o.thr[q];
            for (uint32_t wl = wave; wl < 2u * tcn; wl += kFlatWaves) {
                const uint32_t w = 2u * c0 + wl;
                if (w >= o.W) break;
                const uint32_t at = (wl >> 1) * kLdsPitch + (wl & 1u) * 64u + lane;
                const uint32_t n = lds[at];
                lds[at] = 0;
                const size_t ci = ((size_t)q * W + w) * 64 + lane;
                if (whole) {
                    const bool valid = ((uint64_t)(o.word0 + w) << 6) + lane < o.user_bins;
                    const uint64_t hit = __ballot(valid && n >= t);
                    if (lane == 0) o.hits[(size_t)q * W + w] = hit;
                    if (o.counts) o.counts[ci] = n;
                } else if (n) {
                    atomicAdd(o.acc + ci, n);
                }
            }
            __syncthreads();
            pos = stop;
            if (pos < hi) {
                ++q;
                while (o.offsets[q + 1] <= pos) ++q;  // (empty queries: count_finish_kernel answers them)
            }
        }
    }
}

// Zero the accumulator rows of the queries longer than a unit (before count_flat_kernel adds to them).
__global__ __launch_bounds__(64) void count_zero_long_kernel(CountOut o) {
    const uint64_t base = o.offsets[0], end = o.offsets[o.nq];
    if (end <= base) return;
    const uint64_t seg = seg_len(end - base);
    const size_t row = (size_t)o.W * 64;
    for (uint32_t q = blockIdx.x; q < o.nq; q += gridDim.x)
        if (o.offsets[q + 1] - o.offsets[q] > seg)
            for (size_t i = threadIdx.x; i < row; i += 64) o.acc[(size_t)q * row + i] = 0;
}

// Answer the queries count_flat_kernel did not write: empty ones (count 0) and long ones (from their accumulators).
__global__ __launch_bounds__(64) void count_finish_kernel(CountOut o) {
    const uint32_t lane = threadIdx.x;
    const uint64_t base = o.offsets[0], end = o.offsets[o.nq];
    const uint64_t seg = end > base ? seg_len(end - base) : 0;
    const size_t W = o.W;
    for (uint32_t q = blockIdx.x; q < o.nq; q += gridDim.x) {
        const uint64_t len = o.offsets[q + 1] - o.offsets[q];
        if (len && len <= seg) continue;
        const uint32_t t = o.thr[q];
        for (uint32_t w = 0; w < o.W; ++w) {
            const size_t ci = ((size_t)q * W + w) * 64 + lane;
            const uint32_t n = len ? o.acc[ci] : 0u;
            const bool valid = ((uint64_t)(o.word0 + w) << 6) + lane < o.user_bins;
            const uint64_t hit = __ballot(valid && n >= t);
            if (lane == 0) o.hits[(size_t)q * W + w] = hit;
            if (o.counts && !len) o.counts[ci] = 0;  // (a long query's counts are its accumulators: acc == counts)
        }
    }
}

// ---- flat IBF, sliding windows (txq_count_windows) --------------------------------------------------------------------------
//
// Window j owns values [begin[j], begin[j] + len[j]); the windows slide (begin and begin + len do not decrease).  A workgroup
// of NW waves takes a unit of U consecutive windows and one column tile, and keeps the CURRENT window's counters in LDS:
// cw_step (txq_count_windows_plan.hpp) says which values enter (added) and which leave (subtracted), or that the counters
// start from zero.  u32 arithmetic is modular, so the waves add and subtract concurrently; the counters are read behind a
// barrier, thresholded and written once per (window, word) as count_flat_kernel writes a whole query, and NOT cleared.  A
// leaving row was read at most one window length ago by the same workgroup: it comes from L2.  The leaving pass starts at
// wave NW / 2, so that a step of a few values keeps two waves busy, not one twice.  A window is counted by ONE workgroup.

struct WindowsOut {
    const uint64_t* values;
    const uint64_t* begin;  // n
    const uint32_t* len;    // n
    const uint32_t* thr;    // n
    uint64_t* hits;         // [n][W]
    uint32_t* counts;       // [n][64 W] or null
    uint64_t user_bins;
    uint64_t n;
    uint32_t W, word0, U;
};

template <int H, int NW>
__global__ __launch_bounds__(64 * NW) void count_windows_kernel(IbfDev f, WindowsOut o, uint32_t lpk_log2, uint32_t n_tiles) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
    const uint32_t tile = 1u << lpk_log2;
    const uint32_t lds_words = (chunks < tile ? chunks : tile) * kLdsPitch;
    const uint64_t n_units = cw_units(o.n, o.U);
    const size_t W = o.W;
    for (uint64_t work = blockIdx.x; work < n_units * n_tiles; work += gridDim.x) {
        const uint64_t u = work / n_tiles;
        const uint32_t c0 = (uint32_t)(work % n_tiles) << lpk_log2;
        const uint32_t tcn = chunks - c0 < tile ? chunks - c0 : tile;  // chunks of this tile
        const uint64_t j0 = cw_unit_first(u, o.U), j1 = cw_unit_last(u, o.U, o.n);
        uint64_t pb = 0, pe = 0;
        for (uint64_t j = j0; j < j1; ++j) {
            const uint64_t b = o.begin[j], e = b + o.len[j];
            const CwStep st = cw_step(j == j0, pb, pe, b, e);
            if (st.reset) {  // (the reads of the window before are behind the barrier that ended it)
                for (uint32_t i = threadIdx.x; i < lds_words; i += 64 * NW) lds[i] = 0;
                __syncthreads();
            }
            count_values<H, false>(f, lpk_log2, c0, chunks, o.values, st.add_lo, st.add_hi, lds, wave, NW);
            if (st.sub_lo < st.sub_hi) count_values<H, true>(f, lpk_log2, c0, chunks, o.values, st.sub_lo, st.sub_hi, lds, (wave + NW / 2) % NW, NW);
            __syncthreads();
            const uint32_t t = o.thr[j];
            for (uint32_t wl = wave; wl < 2u * tcn; wl += NW) {
                const uint32_t w = 2u * c0 + wl;
                if (w >= o.W) break;
                const uint32_t n = lds[(wl >> 1) * kLdsPitch + (wl & 1u) * 64u + lane];
                const bool valid = ((uint64_t)(o.word0 + w) << 6) + lane < o.user_bins;
                const uint64_t hit = __ballot(valid && n >= t);
                if (lane == 0) o.hits[(size_t)j * W + w] = hit;
                if (o.counts) o.counts[((size_t)j * W + w) * 64 + lane] = n;
            }
            __syncthreads();
            pb = b, pe = e;
        }
    }
}

// ---- HIBF ---------------------------------------------------------------------------------------------------------------

struct HibfCountView {
    const IbfDev* ibf;
    const uint64_t* next;
    const uint64_t* tb_user;
    const uint64_t* map_off;
    const uint64_t* descend;     // merged bins whose sub-tree holds user bins of this shard's columns
    const uint64_t* merged_off;
};

// One level: work item (query, IBF) per wave.  Level 0 (in == null): (q, root) for q < n_level0.  Every IBF has at most
// 64 chunks (checked at the call), so its whole row of counters is in LDS: max chunks * 129 u32.
template <int H>
__global__ __launch_bounds__(64) void count_hibf_level_kernel(HibfCountView t, CountOut o, const WorkItem* __restrict__ in,
                                                              const uint32_t* __restrict__ in_count, uint32_t in_cap, uint32_t n_level0,
                                                              WorkItem* __restrict__ out, uint32_t* __restrict__ out_count, uint32_t out_cap,
                                                              uint32_t lds_words) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < lds_words; i += 64) lds[i] = 0;
    __syncthreads();
    const uint32_t count = in ? min(*in_count, in_cap) : n_level0;
    const size_t W = o.W;
    unsigned long long t_items = 0, t_added = 0;  // this wave's part of txq_count_windows_trace (o.trace), added once at its end
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t q = in ? in[item].kmer : item;
        const uint32_t id = in ? in[item].ibf : 0u;
        const IbfDev f = t.ibf[id];
        const uint64_t off = t.map_off[id], moff = t.merged_off[id];
        const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
        uint32_t lpk_log2 = 0;
        while ((1u << lpk_log2) < chunks) ++lpk_log2;
        const uint64_t q_lo = o.offsets[q], q_hi = o.lens ? q_lo + o.lens[q] : o.offsets[q + 1];
        count_values<H>(f, lpk_log2, 0, chunks, o.values, q_lo, q_hi, lds);
        __syncthreads();
        const uint32_t thr = o.thr[q];
        for (uint32_t b0 = 0; b0 < f.bins; b0 += 64) {
            const uint32_t tb = b0 + lane;
            const bool live = tb < f.bins;
            const uint32_t n = live ? lds[(tb >> 7) * kLdsPitch + (tb & 127u)] : 0u;
            const uint64_t ub = live ? t.tb_user[off + tb] : 0;
            const bool merged = live && ub == TXQ_MERGED_BIN;
            const bool kid = merged && n >= thr && ((t.descend[moff + (tb >> 6)] >> (tb & 63u)) & 1ULL);
            const uint64_t kids = __ballot(kid);
            if (kids) {  // (query, child) -> next level, one atomic per wave and 64 bins
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(out_count, (uint32_t)__builtin_popcountll(kids));
                at = __shfl(at, 0) + (uint32_t)__builtin_popcountll(kids & ((1ULL << lane) - 1ULL));
                if (kid && at < out_cap) out[at] = WorkItem{q, (uint32_t)t.next[off + tb]};
            }
            if (live && !merged && (tb + 1 == f.bins || t.tb_user[off + tb + 1] != ub)) {  // the last technical bin of a user bin's run
                uint32_t sum = n;
                for (uint32_t s = tb; s > 0 && t.tb_user[off + s - 1] == ub; --s) sum += lds[((s - 1) >> 7) * kLdsPitch + ((s - 1) & 127u)];
                const uint64_t w = ub >> 6;
                if (ub < o.user_bins && w >= o.word0 && w < (uint64_t)o.word0 + o.W) {
                    const size_t wl = (size_t)(w - o.word0);
                    // (a user bin whose parts are not adjacent has several runs: a hit if any passes, its count the largest)
                    if (o.counts) atomicMax(o.counts + ((size_t)q * W + wl) * 64 + (ub & 63), sum);
                    if (sum >= thr) atomicOr((unsigned long long*)(o.hits + (size_t)q * W + wl), 1ULL << (ub & 63));
                }
            }
        }
        ++t_items, t_added += q_hi - q_lo;
        __syncthreads();
        for (uint32_t i = lane; i < chunks * kLdsPitch; i += 64) lds[i] = 0;
        __syncthreads();
    }
    if (o.trace && lane == 0 && t_items) {  // (windows as independent queries: a visit is an item, counted in full)
        unsigned long long* tr = o.trace + (size_t)(blockIdx.x % kCwTraceSlots) * kCwTraceWords;
        atomicAdd(tr + kCwTraceVisits, t_items);
        atomicAdd(tr + kCwTraceAdded, t_added);
        atomicAdd(tr + kCwTraceItems, t_items);
    }
}

// ---- HIBF, sliding windows (txq_count_windows) --------------------------------------------------------------------------------
//
// One level: work item (unit, IBF, mask) per wave (txq_count_windows_tree_plan.hpp).  Level 0 (in == null): (u, root, all
// windows of unit u) for u < n_level0.  The wave walks the item's windows in order and keeps the CURRENT window's counters
// on this IBF in LDS: cw_step between two VISITED windows says which values enter and which leave, or that the counters
// start from zero — always so at the item's first window, since they hold what the wave's last item left.  After each
// window the technical-bin pass of count_hibf_level_kernel runs on the counters; a merged bin that passes appends nothing,
// its lane ORs the window's bit into the bin's mask word (LDS, behind the counters: one lane owns a bin in a pass).  After
// the last window every non-zero mask word becomes the child's item, and is zeroed for the wave's next item.
// LDS: max chunks * 129 u32 counters, then one u32 mask word per technical bin of the widest IBF.

struct WindowsTreeOut {
    const uint64_t* values;
    const uint64_t* begin;       // n (of this device call: it starts at a unit boundary)
    const uint32_t* len;         // n
    const uint32_t* thr;         // n
    uint64_t* hits;              // [n][W]
    uint32_t* counts;            // [n][64 W] or null
    unsigned long long* trace;   // [kCwTraceSlots][kCwTraceWords]: txq_count_windows_trace
    uint64_t user_bins;
    uint64_t n;
    uint32_t W, word0, U;
};

template <int H>
__global__ __launch_bounds__(64) void count_windows_tree_kernel(HibfCountView t, WindowsTreeOut o, const CwTreeItem* __restrict__ in,
                                                                const uint32_t* __restrict__ in_count, uint32_t in_cap, uint32_t n_level0,
                                                                CwTreeItem* __restrict__ out, uint32_t* __restrict__ out_count, uint32_t out_cap,
                                                                uint32_t cnt_words, uint32_t mask_words) {
    extern __shared__ uint32_t lds[];
    uint32_t* kid_mask = lds + cnt_words;
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < mask_words; i += 64) kid_mask[i] = 0;
    __syncthreads();
    const uint32_t count = in ? min(*in_count, in_cap) : n_level0;
    const size_t W = o.W;
    // This wave's part of txq_count_windows_trace, over all of its items: added once, at the wave's end, to one of kCwTraceSlots
    // sets of totals.  (One set that every item adds to costs 10 ns an item on 3 * 10^5 items: the adds to one address queue up.)
    unsigned long long t_visits = 0, t_added = 0, t_subtracted = 0, t_items = 0;
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t unit = in ? in[item].unit : item;
        const uint32_t id = in ? in[item].ibf : 0u;
        const uint32_t mask = in ? in[item].mask : cwt_level0_mask(unit, o.U, o.n);
        const IbfDev f = t.ibf[id];
        const uint64_t off = t.map_off[id], moff = t.merged_off[id];
        const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
        uint32_t lpk_log2 = 0;
        while ((1u << lpk_log2) < chunks) ++lpk_log2;
        const uint64_t j0 = cw_unit_first(unit, o.U);
        uint64_t added = 0, subtracted = 0;
        for (CwTreeWalk wk = cwt_walk(mask); cwt_more(wk);) {
            const uint32_t wi = cwt_window(wk);
            const uint64_t j = j0 + wi;
            const uint64_t b = o.begin[j], e = b + o.len[j];
            const CwStep st = cwt_advance(wk, b, e);
            if (st.reset) {  // (the reads of the window before are behind the barrier that ended it)
                for (uint32_t i = lane; i < chunks * kLdsPitch; i += 64) lds[i] = 0;
                __syncthreads();
            }
            count_values<H, false>(f, lpk_log2, 0, chunks, o.values, st.add_lo, st.add_hi, lds);
            if (st.add_lo < st.add_hi) added += st.add_hi - st.add_lo;
            if (st.sub_lo < st.sub_hi) {
                count_values<H, true>(f, lpk_log2, 0, chunks, o.values, st.sub_lo, st.sub_hi, lds);
                subtracted += st.sub_hi - st.sub_lo;
            }
            __syncthreads();
            const uint32_t thr = o.thr[j];
            for (uint32_t b0 = 0; b0 < f.bins; b0 += 64) {
                const uint32_t tb = b0 + lane;
                const bool live = tb < f.bins;
                const uint32_t n = live ? lds[(tb >> 7) * kLdsPitch + (tb & 127u)] : 0u;
                const uint64_t ub = live ? t.tb_user[off + tb] : 0;
                const bool merged = live && ub == TXQ_MERGED_BIN;
                if (merged && n >= thr && ((t.descend[moff + (tb >> 6)] >> (tb & 63u)) & 1ULL)) kid_mask[tb] |= 1u << wi;
                if (live && !merged && (tb + 1 == f.bins || t.tb_user[off + tb + 1] != ub)) {  // the last technical bin of a user bin's run
                    uint32_t sum = n;
                    for (uint32_t s = tb; s > 0 && t.tb_user[off + s - 1] == ub; --s) sum += lds[((s - 1) >> 7) * kLdsPitch + ((s - 1) & 127u)];
                    const uint64_t w = ub >> 6;
                    if (ub < o.user_bins && w >= o.word0 && w < (uint64_t)o.word0 + o.W) {
                        const size_t wl = (size_t)(w - o.word0);
                        // (a user bin whose parts are not adjacent has several runs: a hit if any passes, its count the largest)
                        if (o.counts) atomicMax(o.counts + ((size_t)j * W + wl) * 64 + (ub & 63), sum);
                        if (sum >= thr) atomicOr((unsigned long long*)(o.hits + (size_t)j * W + wl), 1ULL << (ub & 63));
                    }
                }
            }
            __syncthreads();  // (the next window changes the counters the run sums read)
        }
        for (uint32_t b0 = 0; b0 < f.bins; b0 += 64) {  // (unit, child, windows that descend) -> next level, one atomic per wave and 64 bins
            const uint32_t tb = b0 + lane;
            const uint32_t m = tb < f.bins ? kid_mask[tb] : 0u;
            const uint64_t kids = __ballot(m != 0);
            if (kids) {
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(out_count, (uint32_t)__builtin_popcountll(kids));
                at = __shfl(at, 0) + (uint32_t)__builtin_popcountll(kids & ((1ULL << lane) - 1ULL));
                if (m) {
                    if (at < out_cap) out[at] = CwTreeItem{unit, (uint32_t)t.next[off + tb], m};
                    kid_mask[tb] = 0;
                }
            }
        }
        t_visits += (unsigned long long)__builtin_popcount(mask), t_added += added, t_subtracted += subtracted, ++t_items;  // the item's totals, once
        __syncthreads();
    }
    if (lane == 0 && t_items) {
        unsigned long long* tr = o.trace + (size_t)(blockIdx.x % kCwTraceSlots) * kCwTraceWords;
        atomicAdd(tr + kCwTraceVisits, t_visits);
        atomicAdd(tr + kCwTraceAdded, t_added);
        atomicAdd(tr + kCwTraceSubtracted, t_subtracted);
        atomicAdd(tr + kCwTraceItems, t_items);
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------

static int count_flat(Index& ix, CountOut o, hipStream_t s) {
    const IbfDev& f = ix.ibf[0];
    const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
    uint32_t lpk_log2 = 0;
    while ((1u << lpk_log2) < std::min(chunks, kTileChunks)) ++lpk_log2;
    const uint32_t n_tiles = (chunks + kTileChunks - 1) / kTileChunks;
    const size_t lds = (size_t)std::min(chunks, 1u << lpk_log2) * kLdsPitch * 4;
    const size_t row = (size_t)o.W * 64;
    // long queries add their partial counts to a row of u32 per query: the caller's counts, or scratch of a bounded number
    // of queries at a time
    const size_t per_call = o.counts ? o.nq : count_flat_per_call(o.nq, row);
    if (!o.counts)
        if (int rc = reserved(ix.scratch_count_acc.reserve(exactly(per_call * row * 4), after_device_wait()), "hipMalloc(scratch)")) return rc;
    for (size_t q0 = 0; q0 < o.nq; q0 += per_call) {
        CountOut c = o;
        c.nq = (uint32_t)std::min(per_call, (size_t)o.nq - q0);
        c.offsets = o.offsets + q0;
        c.thr = o.thr + q0;
        c.hits = o.hits + q0 * o.W;
        c.counts = o.counts ? o.counts + q0 * row : nullptr;
        c.acc = o.counts ? c.counts : ix.scratch_count_acc.get();
        const unsigned qgrid = (unsigned)std::min<size_t>(c.nq, kCountGrid);
        count_zero_long_kernel<<<qgrid, 64, 0, s>>>(c);
        if (!with_hash_funs(f.hash_funs, [&](auto h) { count_flat_kernel<decltype(h)::value><<<kCountGrid, 64 * kFlatWaves, lds, s>>>(f, c, lpk_log2, n_tiles); }))
            return fail(TXQ_ERR_ARG, "hash_funs outside 1..5");
        count_finish_kernel<<<qgrid, 64, 0, s>>>(c);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(e, "count kernel launch");
    }
    return TXQ_OK;
}

static int count_hibf(Index& ix, CountOut o, hipStream_t s) {
    uint32_t max_chunks = 1, h_max = 1;
    for (const IbfDev& f : ix.ibf) {
        const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
        if (chunks > kTileChunks) return fail(TXQ_ERR_ARG, "txq_count: an IBF of the tree has more than %u technical bins", kTileChunks * 128);
        max_chunks = std::max(max_chunks, chunks);
        h_max = std::max(h_max, f.hash_funs);
    }
    const size_t row = (size_t)o.W * 64;
    TXQ_HIP(hipMemsetAsync(o.hits, 0, (size_t)o.nq * o.W * 8, s));
    if (o.counts) TXQ_HIP(hipMemsetAsync(o.counts, 0, (size_t)o.nq * row * 4, s));
    // a (query, IBF) pair occurs at most once: level l holds at most chunk * (IBFs on level l) items
    const size_t chunk = count_hibf_chunk(o.nq, ix.max_level_width);
    const size_t cap = chunk * ix.max_level_width;
    if (ix.depth > 1)
        for (int i = 0; i < 2; ++i)
            if (int rc = reserved(ix.frontier[i].reserve(exactly(cap * sizeof(WorkItem)), after_device_wait()), "hipMalloc(scratch)")) return rc;
    if (int rc = reserved(ix.d_counts.reserve(exactly(((size_t)ix.depth + 2) * 4), after_device_wait()), "hipMalloc(scratch)")) return rc;
    const HibfCountView t{ix.d_ibf, ix.d_next, ix.d_tb_user, ix.d_map_off, ix.d_descend, ix.d_merged_off};
    const uint32_t lds_words = max_chunks * kLdsPitch;
    for (size_t q0 = 0; q0 < o.nq; q0 += chunk) {
        CountOut c = o;
        c.nq = (uint32_t)std::min(chunk, (size_t)o.nq - q0);
        c.offsets = o.offsets + q0;
        c.lens = o.lens ? o.lens + q0 : nullptr;
        c.thr = o.thr + q0;
        c.hits = o.hits + q0 * o.W;
        c.counts = o.counts ? o.counts + q0 * row : nullptr;
        TXQ_HIP(hipMemsetAsync(ix.d_counts.get(), 0, ((size_t)ix.depth + 2) * 4, s));
        for (uint32_t lvl = 0; lvl < ix.depth; ++lvl) {
            const WorkItem* in = lvl ? ix.frontier[(lvl - 1) & 1].get() : nullptr;
            const uint32_t* in_count = lvl ? ix.d_counts.get() + (lvl - 1) : nullptr;
            WorkItem* out = ix.frontier[lvl & 1].get();
            const uint32_t out_cap = ix.depth > 1 && lvl + 1 < ix.depth ? (uint32_t)cap : 0u;
            const unsigned grid = lvl ? kCountGrid : (unsigned)std::min<size_t>(c.nq, kCountGrid);
            if (!with_hash_funs(h_max, [&](auto h) {
                    count_hibf_level_kernel<decltype(h)::value><<<grid, 64, lds_words * 4, s>>>(t, c, in, in_count, (uint32_t)cap, c.nq, out, ix.d_counts.get() + lvl,
                                                                                                out_cap, lds_words);
                }))
                return fail(TXQ_ERR_ARG, "hash_funs outside 1..5");
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail_hip(e, "hibf count kernel launch");
        }
    }
    return TXQ_OK;
}

int count_device(Index& ix, const uint64_t* d_values, const uint64_t* d_offsets, size_t n_queries, const uint32_t* d_thr,
                 uint64_t* d_hits, uint32_t* d_counts, hipStream_t s) {
    if (n_queries == 0 || ix.shard_words == 0) return TXQ_OK;
    CountOut o{};
    o.values = d_values;
    o.offsets = d_offsets;
    o.thr = d_thr;
    o.hits = d_hits;
    o.counts = d_counts;
    o.acc = d_counts;
    o.user_bins = ix.user_bins;
    o.nq = (uint32_t)n_queries;
    o.W = (uint32_t)ix.shard_words;
    o.word0 = (uint32_t)ix.shard_word0;
    return ix.is_hibf ? count_hibf(ix, o, s) : count_flat(ix, o, s);
}

static int count_windows_flat(Index& ix, WindowsOut o, hipStream_t s) {
    const IbfDev& f = ix.ibf[0];
    const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
    uint32_t lpk_log2 = 0;
    while ((1u << lpk_log2) < std::min(chunks, kTileChunks)) ++lpk_log2;
    const uint32_t n_tiles = (chunks + kTileChunks - 1) / kTileChunks;
    const size_t lds = (size_t)std::min(chunks, 1u << lpk_log2) * kLdsPitch * 4;
    o.U = env_u32("TXQ_COUNT_WINDOWS_UNIT", kCountWindowsUnitDefault, 1, kCountWindowsUnitMax);
    const uint32_t waves = env_u32("TXQ_COUNT_WINDOWS_WAVES", kWindowsWaves, 1, 4) >= 4 ? 4 : 1;
    const unsigned grid = (unsigned)std::min<uint64_t>(cw_units(o.n, o.U) * n_tiles, (uint64_t)kCountGrid * 4);
    const bool ok = with_hash_funs(f.hash_funs, [&](auto h) {
        if (waves == 4) count_windows_kernel<decltype(h)::value, 4><<<grid, 256, lds, s>>>(f, o, lpk_log2, n_tiles);
        else count_windows_kernel<decltype(h)::value, 1><<<grid, 64, lds, s>>>(f, o, lpk_log2, n_tiles);
    });
    if (!ok) return fail(TXQ_ERR_ARG, "hash_funs outside 1..5");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "count windows kernel launch");
    return TXQ_OK;
}

// The totals of txq_count_windows_trace start from zero on the call's stream; `done` is recorded behind the call's last kernel.
static int count_windows_trace_begin(Index& ix, hipStream_t s) {
    Index::CountWindowsTrace& tr = ix.count_windows_trace;
    if (int rc = reserved(tr.totals.reserve(exactly(kCwTraceSlots * kCwTraceWords * sizeof(unsigned long long)), after_device_wait()), "hipMalloc(scratch)")) return rc;
    TXQ_HIP(make(tr.done));
    TXQ_HIP(hipMemsetAsync(tr.totals.get(), 0, kCwTraceSlots * kCwTraceWords * sizeof(unsigned long long), s));
    return TXQ_OK;
}

static int count_windows_tree(Index& ix, WindowsTreeOut o, hipStream_t s) {
    uint32_t max_chunks = 1, h_max = 1, max_bins = 1;
    for (const IbfDev& f : ix.ibf) {
        const uint32_t chunks = f.stride == 1 ? 1u : f.stride >> 1;
        if (chunks > kTileChunks) return fail(TXQ_ERR_ARG, "txq_count: an IBF of the tree has more than %u technical bins", kTileChunks * 128);
        max_chunks = std::max(max_chunks, chunks);
        max_bins = std::max(max_bins, (uint32_t)f.bins);
        h_max = std::max(h_max, f.hash_funs);
    }
    o.U = cwt_unit(env_u32("TXQ_COUNT_WINDOWS_UNIT", kCountWindowsUnitDefault, 1, kCountWindowsUnitMax));
    const size_t row = (size_t)o.W * 64;
    TXQ_HIP(hipMemsetAsync(o.hits, 0, (size_t)o.n * o.W * 8, s));
    if (o.counts) TXQ_HIP(hipMemsetAsync(o.counts, 0, (size_t)o.n * row * 4, s));
    const size_t n_units = (size_t)cw_units(o.n, o.U);
    const size_t per_call = cwt_units_per_call(n_units, ix.max_level_width, kHibfCapItems);
    const size_t cap = cwt_frontier_items(per_call, ix.max_level_width);
    if (ix.depth > 1)
        for (int i = 0; i < 2; ++i)
            if (int rc = reserved(ix.frontier[i].reserve(exactly(cap * sizeof(CwTreeItem)), after_device_wait()), "hipMalloc(scratch)")) return rc;
    if (int rc = reserved(ix.d_counts.reserve(exactly(((size_t)ix.depth + 2) * 4), after_device_wait()), "hipMalloc(scratch)")) return rc;
    const HibfCountView t{ix.d_ibf, ix.d_next, ix.d_tb_user, ix.d_map_off, ix.d_descend, ix.d_merged_off};
    const uint32_t cnt_words = max_chunks * kLdsPitch, mask_words = (max_bins + 63u) / 64u * 64u;
    const size_t lds_bytes = ((size_t)cnt_words + mask_words) * 4;
    if (lds_bytes > (48u << 10)) {  // (more dynamic LDS than the default limit: ask for it, once per call)
        hipError_t e = hipSuccess;
        if (!with_hash_funs(h_max, [&](auto h) {
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(&count_windows_tree_kernel<decltype(h)::value>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            }))
            return fail(TXQ_ERR_ARG, "hash_funs outside 1..5");
        if (e != hipSuccess) return fail_hip(e, "hipFuncSetAttribute");
    }
    for (size_t u0 = 0; u0 < n_units; u0 += per_call) {  // device calls are cut at unit boundaries
        const size_t j0 = (size_t)cw_unit_first(u0, o.U), nu = std::min(per_call, n_units - u0);
        WindowsTreeOut c = o;
        c.n = std::min<uint64_t>((uint64_t)nu * o.U, o.n - j0);
        c.begin = o.begin + j0;
        c.len = o.len + j0;
        c.thr = o.thr + j0;
        c.hits = o.hits + j0 * o.W;
        c.counts = o.counts ? o.counts + j0 * row : nullptr;
        TXQ_HIP(hipMemsetAsync(ix.d_counts.get(), 0, ((size_t)ix.depth + 2) * 4, s));
        for (uint32_t lvl = 0; lvl < ix.depth; ++lvl) {
            const CwTreeItem* in = lvl ? reinterpret_cast<const CwTreeItem*>(ix.frontier[(lvl - 1) & 1].get()) : nullptr;
            const uint32_t* in_count = lvl ? ix.d_counts.get() + (lvl - 1) : nullptr;
            CwTreeItem* out = reinterpret_cast<CwTreeItem*>(ix.frontier[lvl & 1].get());
            const uint32_t out_cap = ix.depth > 1 && lvl + 1 < ix.depth ? (uint32_t)cap : 0u;
            const unsigned grid = lvl ? kCountGrid : (unsigned)std::min<size_t>(nu, kCountGrid);
            if (!with_hash_funs(h_max, [&](auto h) {
                    count_windows_tree_kernel<decltype(h)::value><<<grid, 64, lds_bytes, s>>>(t, c, in, in_count, (uint32_t)cap, (uint32_t)nu, out, ix.d_counts.get() + lvl,
                                                                                              out_cap, cnt_words, mask_words);
                }))
                return fail(TXQ_ERR_ARG, "hash_funs outside 1..5");
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail_hip(e, "hibf count windows kernel launch");
        }
    }
    return TXQ_OK;
}

int count_windows_device(Index& ix, const uint64_t* d_values, const uint64_t* d_begin, const uint32_t* d_len, size_t n_windows,
                         const uint32_t* d_thr, uint64_t* d_hits, uint32_t* d_counts, hipStream_t s) {
    if (ix.is_hibf) ix.count_windows_trace.recorded = false;  // (a call of no windows, or one that fails: txq_count_windows_trace reports zeros, not the call before)
    if (n_windows == 0 || ix.shard_words == 0) return TXQ_OK;
    if (ix.is_hibf) {
        if (int rc = count_windows_trace_begin(ix, s)) return rc;
        Index::CountWindowsTrace& tr = ix.count_windows_trace;
        int rc = TXQ_OK;
        if (env_u32("TXQ_COUNT_WINDOWS_TREE", kCountWindowsTreeDefault, 0, 1)) {  // sliding: a wave per (unit of windows, IBF)
            WindowsTreeOut o{};
            o.values = d_values;
            o.begin = d_begin;
            o.len = d_len;
            o.thr = d_thr;
            o.hits = d_hits;
            o.counts = d_counts;
            o.trace = tr.totals.get();
            o.user_bins = ix.user_bins;
            o.n = n_windows;
            o.W = (uint32_t)ix.shard_words;
            o.word0 = (uint32_t)ix.shard_word0;
            rc = count_windows_tree(ix, o, s);
        } else {  // the windows as independent queries: each (window, IBF) pair counted in full by one wave, no sliding
            CountOut o{};
            o.values = d_values;
            o.offsets = d_begin;
            o.lens = d_len;
            o.thr = d_thr;
            o.hits = d_hits;
            o.counts = d_counts;
            o.acc = d_counts;
            o.trace = tr.totals.get();
            o.user_bins = ix.user_bins;
            o.nq = (uint32_t)n_windows;
            o.W = (uint32_t)ix.shard_words;
            o.word0 = (uint32_t)ix.shard_word0;
            rc = count_hibf(ix, o, s);
        }
        if (rc) return rc;
        TXQ_HIP(hipEventRecord(tr.done.get(), s));
        tr.recorded = true;
        return TXQ_OK;
    }
    WindowsOut o{};
    o.values = d_values;
    o.begin = d_begin;
    o.len = d_len;
    o.thr = d_thr;
    o.hits = d_hits;
    o.counts = d_counts;
    o.user_bins = ix.user_bins;
    o.n = n_windows;
    o.W = (uint32_t)ix.shard_words;
    o.word0 = (uint32_t)ix.shard_word0;
    return count_windows_flat(ix, o, s);
}

}  // namespace txq
