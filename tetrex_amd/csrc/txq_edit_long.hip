// Approximate matching of (pattern, bin) pairs by edit distance on gfx950, patterns of up to 4096 bytes
// (txq_edit_search_long / txq_edit_search_long_device; `tetrex search --verify` for records of 513 .. 4096 letters, DESIGN.md
// §12 "Long patterns").  The semantics are those of txq_edit_search_device in include/txq.h.
//
// txq_edit.hip gives every lane the whole pattern and a chunk of the text; at m = 4096 that would be 128 state words per
// lane and a lead-in of eight default chunks.  Here the pattern lies over the lanes of a wave and the text is walked once,
// as a systolic array (the step logic and its exactness: txq_edit_long_plan.hpp, which the CPU test runs as well):
//   * a pattern of W = ceil(m / 64) words runs on a group of G lanes, G the smallest of 16, 32, 64 with G >= W; lane w of
//     the group keeps Pv / Mv of word w in two 64-bit VGPR values, lanes >= W idle.  A wave carries 64 / G groups, each on
//     its own span of the same pair's text, so the wave builds one Peq table per unit;
//   * at step s lane w works on text column s - w.  One cross-lane move per step — a DPP shift of the wave by one lane, no
//     LDS round trip — hands it the message lane w - 1 made one step earlier: the column's class, its horizontal delta and
//     the flag "a record begins here", which resets Pv / Mv in every lane it passes and the score in the lane of row m - 1.
//     Lane 0 of a group takes hin = 0 and the next text byte instead of what the shift brings from the group before;
//   * Peq[class][word] lives in LDS, 32 rows of G words (row 31 stays zero): 16 KiB at G = 64, next to the 256-byte class
//     table; lane w reads peq[class * G + w], 8 bytes;
//   * the lane that holds word (m - 1) >> 6 follows the score at bit (m - 1) & 63 and records a key only for columns of its
//     group's own span [ca, cb) and only where the score is within the cap.  The span starts fresh at long_start(): the
//     lead-in argument of txq_edit.hip;
//   * lane 0 of a group loads the text in 16-byte blocks (load_block: nothing outside the text is read); the groups of a
//     wave walk from 16-byte aligned addresses, so that the step loop and its block loads are uniform over the wave, which
//     the cross-lane move needs.  Bytes in front of a group's start and behind its span are columns of no message;
//   * units, prefix, persistent grid, keys, atomicMin per unit and the finish step are those of txq_edit.hip
//     (txq_edit_common.hpp); a unit is one wave's 64 / G spans of TXQ_EDIT_LONG_SPAN bytes.
// Three instances (G = 16, 32, 64), one launch each: a unit whose pattern runs on another group size is skipped.
#include "txq_edit_long_plan.hpp"
#include "txq_scan.hpp"

namespace txq {
namespace {

constexpr uint32_t kMaxPattern = TXQ_EDIT_LONG_MAX_PATTERN;
static_assert(kMaxPattern == kEditLongMaxPattern && kMaxPattern == 64 * 64, "one word per lane");
constexpr uint32_t kDefaultSpan = 4096, kMinSpan = 16, kMaxSpan = 1u << 20;
constexpr uint32_t kGridBlocks = 256 * 16;  // waves of the persistent grid: 16 per CU

__global__ __launch_bounds__(256) void edit_long_plan_kernel(EdArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) a.pref[0] = 0;
    if (i >= a.n_pairs) return;
    const PairView v = view_pair<kMaxPattern>(a, i);
    uint64_t units = 0, key = kBadPair;
    if (v.ok) {
        units = long_units(v.ge - v.gs, long_group_lanes(v.m), a.chunk);
        // end 0 of the group's first record: distance m, the lowest position there is
        key = v.r1 > v.r0 && v.m <= v.e ? (uint64_t)v.m << kPosBits : kNoKey;
    }
    a.pref[i + 1] = units;
    a.keys[i] = key;
}

// every lane gets the value of the lane below it in the wave (lane 0: 0).  Called where all 64 lanes are active.
__device__ __forceinline__ uint32_t from_lane_before(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

template <int G>
__global__ __launch_bounds__(64) void edit_long_kernel(EdArgs a) {
    __shared__ uint64_t peq[32 * G];
    __shared__ uint8_t codes[256];
    const uint32_t lane = threadIdx.x, w = lane % G, group = lane / G;
    const uint64_t total = a.pref[a.n_pairs];
    if (blockIdx.x >= total) return;
    for (uint32_t i = lane; i < 256; i += 64) {
        const uint8_t c = a.codes[i];
        codes[i] = c < 31 ? c : (uint8_t)31;
    }
    const uintptr_t text_lo = (uintptr_t)a.t.text, text_hi = text_lo + a.t.text_bytes;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t pair = pair_of_unit(a.pref, a.n_pairs, u);
        const PairView v = view_pair<kMaxPattern>(a, pair);
        if (!v.ok || long_group_lanes(v.m) != (uint32_t)G) continue;  // (uniform over the wave)
        const uint64_t slice = u - a.pref[pair];
        __syncthreads();  // the unit before is done with peq
        for (uint32_t i = lane; i < 32 * G; i += 64) peq[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < v.m; i += 64) {
            const uint32_t c = codes[a.pat[v.p0 + i]];
            if (c < 31) atomicOr(reinterpret_cast<uint32_t*>(peq) + 2 * (c * G + (i >> 6)) + ((i >> 5) & 1), 1u << (i & 31));
        }
        __syncthreads();

        const uint32_t m = v.m, e = v.e;
        const uint32_t hw = (m - 1) >> 6, bit = w == hw ? (m - 1) & 63 : 63u;
        const auto [ca, cb] = long_span(v.gs, v.ge, slice, G, group, a.chunk);
        // this group's walk: columns from the 16-byte block that holds `start` up to cb, column c being byte t0 + c of the
        // text (t0 + c wraps to the true index where the block begins below the text: load_block)
        uint64_t start = 0, t0 = 0, columns = 0, rf = v.r0, rf_end = 0;
        uintptr_t base = 0;
        if (ca < v.ge) {
            rf = record_of(a.t.rec, v.r0, v.r1, ca);
            rf_end = a.t.rec[rf + 1];
            start = long_start(ca, a.t.rec[rf], v.gs, m, e);
            base = (text_lo + start) & ~(uintptr_t)15;
            t0 = (uint64_t)(base - text_lo);
            columns = (uint64_t)(text_lo + cb - base);
        }
        uint64_t steps = long_steps(columns, m);  // the most of the wave's groups
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t o = __shfl_xor(steps, d);
            steps = o > steps ? o : steps;
        }
        uint64_t pv = ~0ULL, mv = 0, rs = rf, best = kNoKey;  // (rs: the record of the scoring lane's column)
        uint32_t score = m, out = 0;
        for (uint64_t s0 = 0; s0 < steps; s0 += 16) {
            TextBlock raw{};
            if (w == 0 && s0 < columns) raw = load_block(base + s0, text_lo, text_hi, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t word = raw.w[q];
#pragma nounroll
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint64_t s = s0 + 4u * q + b;
                    uint32_t msg = from_lane_before(out);
                    if (w == 0) {  // the next text byte, where this group has one
                        const uint64_t t = t0 + s;
                        msg = 0;
                        if (s < columns && t >= start && t < cb) {
                            const bool reset = t >= rf_end;  // the record ended: a fresh state in the next one that has bytes
                            if (reset) rf_end = long_next_record(a.t.rec, rf, v.r1, v.ge, t);
                            msg = long_feed(codes[(word >> (8 * b)) & 255u], reset);
                        }
                    }
                    out = long_block_step(pv, mv, peq[(msg & kMsgClass) * G + w], msg, bit);
                    if (w == hw && (out & kMsgValid)) {
                        const uint64_t t = t0 + s - hw;
                        if (out & kMsgReset) {
                            score = m;
                            (void)long_next_record(a.t.rec, rs, v.r1, v.ge, t);
                        }
                        score += (uint32_t)long_hin(out);
                        if (t >= ca && score <= e) {
                            const uint64_t key = edit_key(score, t, v.gs, rs, v.r0);
                            best = key < best ? key : best;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t o = __shfl_xor(best, d);
            best = o < best ? o : best;
        }
        if (lane == 0 && best != kNoKey) atomicMin((unsigned long long*)(a.keys + pair), (unsigned long long)best);
    }
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_edit_search_long_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                                const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                                const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                                const uint8_t* d_codes, uint32_t* d_out, void* d_workspace, void* stream) {
    if (int rc = edit_device_args(d_patterns, d_pat_offsets, pattern_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, d_pairs, n_pairs,
                                  d_codes, d_out, d_workspace))
        return rc;
    if (n_pairs == 0) return TXQ_OK;
    hipStream_t st = (hipStream_t)stream;
    void* scratch = d_workspace;  // keys and prefix: TXQ_EDIT_LONG_WORKSPACE(n_pairs) bytes of the caller's
    const uint32_t span = (env_u32("TXQ_EDIT_LONG_SPAN", kDefaultSpan, kMinSpan, kMaxSpan) + 15) / 16 * 16;
    const EdArgs a{d_patterns, d_pat_offsets, n_patterns, pattern_bytes, {d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, n_groups},
                   d_pairs, n_pairs, d_codes, d_out, (uint64_t*)scratch, (uint64_t*)scratch + n_pairs, span};
    const unsigned per_pair = (unsigned)((n_pairs + 255) / 256);
    edit_long_plan_kernel<<<per_pair, 256, 0, st>>>(a);
    scan_kernel<<<1, 1024, 0, st>>>(a.pref + 1, n_pairs);
    edit_long_kernel<16><<<kGridBlocks, 64, 0, st>>>(a);
    edit_long_kernel<32><<<kGridBlocks, 64, 0, st>>>(a);
    edit_long_kernel<64><<<kGridBlocks, 64, 0, st>>>(a);
    edit_finish_kernel<kMaxPattern><<<per_pair, 256, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "long edit kernel launch");
    return TXQ_OK;
}

int txq_edit_search_long(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                         size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                         const uint8_t* codes, uint32_t* out) {
    return edit_search_staged(patterns, pat_offsets, n_patterns, text, rec_offsets, n_records, group_offsets, n_groups, pairs, n_pairs, codes, out,
                              kMaxPattern, TXQ_EDIT_LONG_WORKSPACE(n_pairs), txq_edit_search_long_device, "txq_edit_search_long copies");
}

}  // extern "C"
