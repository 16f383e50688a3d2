// Approximate matching of (pattern, bin) pairs by edit distance on gfx950 (txq_edit_search / txq_edit_search_device;
// `tetrex search --verify`).  The reference has no counterpart.  The semantics are in include/txq.h.
//
// Myers' bit-parallel form of Sellers' recurrence, the pattern ONE integer of W = 1, 2, 4 or 8 words of 64 bits (m <= 64 W):
// the vertical deltas Pv / Mv live in VGPRs, the loops over the words are unrolled at compile time (no array is indexed at
// run time, nothing spills), the addition's carry and the two shifts run from word to word, and the score is followed at bit
// m - 1 (a select over the upper words, since m need not fill the last one).
//
// Mapping to the machine:
//   * a pair's text is the bytes of its group's records, back to back.  edit_plan_kernel cuts it into units of 64 lane
//     chunks of `chunk` bytes (TXQ_EDIT_CHUNK) and scan_kernel (txq_scan.hpp) turns the pairs' unit counts into a prefix: the grid of
//     edit_kernel is persistent, a workgroup of one wave takes units u = block, block + grid, ... and finds (pair, slice) by a
//     binary search in the prefix.  Keys and prefix live in the caller's workspace: the call allocates nothing, reads nothing
//     back and waits for nothing;
//   * per unit the wave builds the pattern's match vectors Peq[class][word] in LDS (32 rows: row 31 stays zero and serves
//     every byte of no class), 2 KiB at most, next to the 256-byte class table;
//   * a lane owns the `chunk` bytes [a, b) of the text.  It starts the recurrence fresh (Pv all ones, Mv zero, score m) at
//     max(record start, a - (m + min(e, m))) and only records scores at bytes of its own chunk.  Exact for every D[m][j] <= e:
//     an alignment of cost <= e that ends at j begins no earlier than j - m - e + 1, and a later start only raises the
//     value.  At a record's end the state is reset;
//   * the text comes in 16-byte loads (byte loads only where the 16 bytes would leave the buffer: txq_text.hpp load_block);
//   * a result is one 64-bit key: distance << 48 | position, the position of end j of record r being (bytes of the group
//     before r) + (records of the group before r) + j, so records and ends are ordered as the contract orders them and j = 0
//     of a record differs from the end of the record before.  Lane minimum, wave minimum (shuffles), one atomicMin per unit;
//     j = 0 (distance m) is put in by the plan kernel where m <= e.  edit_finish_kernel turns keys into (d, r, j).
// Four instances (W = 1, 2, 4, 8), one launch each: a unit whose pattern has another word count is skipped.
#include "txq_edit_common.hpp"
#include "txq_scan.hpp"

namespace txq {
namespace {

constexpr uint32_t kMaxPattern = TXQ_EDIT_MAX_PATTERN;
constexpr uint32_t kDefaultChunk = 512, kMinChunk = 16, kMaxChunk = 1u << 20;
constexpr uint32_t kGridBlocks = 256 * 16;  // waves of the persistent grid: 16 per CU

__device__ __forceinline__ uint32_t words_of(uint32_t m) { return m <= 64 ? 1u : m <= 128 ? 2u : m <= 256 ? 4u : 8u; }

__global__ __launch_bounds__(256) void edit_plan_kernel(EdArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) a.pref[0] = 0;
    if (i >= a.n_pairs) return;
    const PairView v = view_pair<kMaxPattern>(a, i);
    uint64_t units = 0, key = kBadPair;
    if (v.ok) {
        units = units_of(v.ge - v.gs, 64, a.chunk);
        // end 0 of the group's first record: distance m, the lowest position there is
        key = v.r1 > v.r0 && v.m <= v.e ? (uint64_t)v.m << kPosBits : kNoKey;
    }
    a.pref[i + 1] = units;
    a.keys[i] = key;
}

template <int W>
__global__ __launch_bounds__(64) void edit_kernel(EdArgs a) {
    __shared__ uint64_t peq[32 * W];
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
        const uint64_t pair = pair_of_unit(a.pref, a.n_pairs, u);
        const PairView v = view_pair<kMaxPattern>(a, pair);
        if (!v.ok || words_of(v.m) != (uint32_t)W) continue;  // (uniform over the wave)
        const uint64_t slice = u - a.pref[pair];
        __syncthreads();  // the unit before is done with peq
        for (uint32_t i = lane; i < 32 * W; i += 64) peq[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < v.m; i += 64) {
            const uint32_t c = codes[a.pat[v.p0 + i]];
            if (c < 31) atomicOr(reinterpret_cast<uint32_t*>(peq) + 2 * (c * W + (i >> 6)) + ((i >> 5) & 1), 1u << (i & 31));
        }
        __syncthreads();

        const uint32_t m = v.m, e = v.e;
        const uint32_t hw = (m - 1) >> 6, hs = (m - 1) & 63;
        const uint64_t lead = (uint64_t)m + (e < m ? e : m);
        const auto [ca, cb] = chunk_bounds(v.gs, v.ge, slice, 64, lane, a.chunk);
        uint64_t best = kNoKey;
        if (ca < v.ge) {
            uint64_t r = record_of(a.t.rec, v.r0, v.r1, ca);
            uint64_t rs = a.t.rec[r], re = a.t.rec[r + 1];
            // (offsets that do not ascend cannot take a load outside [gs, ge): every byte index below stays in [start, cb))
            if (rs < v.gs || rs > ca) rs = ca;
            const uint64_t start = ca - rs > lead ? ca - lead : rs;
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
                        if (t >= re) {  // the record ended: a fresh state in the next one that has bytes
                            do {
                                ++r;
                                re = r + 1 <= v.r1 ? a.t.rec[r + 1] : v.ge;
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
                            const uint64_t key = (uint64_t)score << kPosBits | (t - v.gs + 1 + (r - v.r0));
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

int txq_edit_search_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                           const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                           const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                           const uint8_t* d_codes, uint32_t* d_out, void* d_workspace, void* stream) {
    if (int rc = edit_device_args(d_patterns, d_pat_offsets, pattern_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, d_pairs, n_pairs,
                                  d_codes, d_out, d_workspace))
        return rc;
    if (n_pairs == 0) return TXQ_OK;
    hipStream_t st = (hipStream_t)stream;
    void* scratch = d_workspace;  // keys and prefix: TXQ_EDIT_WORKSPACE(n_pairs) bytes of the caller's
    const uint32_t chunk = (env_u32("TXQ_EDIT_CHUNK", kDefaultChunk, kMinChunk, kMaxChunk) + 15) / 16 * 16;
    const EdArgs a{d_patterns, d_pat_offsets, n_patterns, pattern_bytes, {d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, n_groups},
                   d_pairs, n_pairs, d_codes, d_out, (uint64_t*)scratch, (uint64_t*)scratch + n_pairs, chunk};
    const unsigned per_pair = (unsigned)((n_pairs + 255) / 256);
    edit_plan_kernel<<<per_pair, 256, 0, st>>>(a);
    scan_kernel<<<1, 1024, 0, st>>>(a.pref + 1, n_pairs);
    edit_kernel<1><<<kGridBlocks, 64, 0, st>>>(a);
    edit_kernel<2><<<kGridBlocks, 64, 0, st>>>(a);
    edit_kernel<4><<<kGridBlocks, 64, 0, st>>>(a);
    edit_kernel<8><<<kGridBlocks, 64, 0, st>>>(a);
    edit_finish_kernel<kMaxPattern><<<per_pair, 256, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "edit kernel launch");
    return TXQ_OK;
}

int txq_edit_search(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                    size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                    const uint8_t* codes, uint32_t* out) {
    return edit_search_staged(patterns, pat_offsets, n_patterns, text, rec_offsets, n_records, group_offsets, n_groups, pairs, n_pairs, codes, out,
                              kMaxPattern, TXQ_EDIT_WORKSPACE(n_pairs), txq_edit_search_device, "txq_edit_search copies");
}

}  // extern "C"
