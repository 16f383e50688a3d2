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
//   * the text comes in 16-byte loads (byte loads only where the 16 bytes would leave the buffer);
//   * a result is one 64-bit key: distance << 48 | position, the position of end j of record r being (bytes of the group
//     before r) + (records of the group before r) + j, so records and ends are ordered as the contract orders them and j = 0
//     of a record differs from the end of the record before.  Lane minimum, wave minimum (shuffles), one atomicMin per unit;
//     j = 0 (distance m) is put in by the plan kernel where m <= e.  edit_finish_kernel turns keys into (d, r, j).
// Four instances (W = 1, 2, 4, 8), one launch each: a unit whose pattern has another word count is skipped.
#include "../../include/txq.h"
#include "txq_internal.hpp"
#include "txq_scan.hpp"

#include <cstdlib>
#include <vector>

namespace txq {
namespace {

constexpr uint32_t kMaxPattern = TXQ_EDIT_MAX_PATTERN;
constexpr uint32_t kDefaultChunk = 512, kMinChunk = 16, kMaxChunk = 1u << 20;
constexpr uint32_t kGridBlocks = 256 * 16;  // waves of the persistent grid: 16 per CU
constexpr uint64_t kNoKey = ~0ULL;
constexpr uint64_t kBadPair = ~0ULL - 1;    // a pair the plan kernel refused
constexpr uint32_t kPosBits = 48;

typedef uint32_t ed4 __attribute__((ext_vector_type(4)));

struct EdArgs {
    const uint8_t* pat;
    const uint64_t* pat_off;
    uint64_t n_pat, pat_bytes;
    const uint8_t* text;
    const uint64_t* rec;
    uint64_t n_rec, text_bytes;
    const uint64_t* grp;
    uint64_t n_grp;
    const uint32_t* pairs;
    uint64_t n_pairs;
    const uint8_t* codes;
    uint32_t* out;
    uint64_t* keys;  // n_pairs
    uint64_t* pref;  // n_pairs + 1: pref[0] = 0, pref[i + 1] = units of pairs 0 .. i
    uint32_t chunk;
};

// What a pair works on; ok = false: an index or an offset outside its array, m = 0 or m > kMaxPattern.
struct PairView {
    bool ok;
    uint32_t m, e;
    uint64_t p0, r0, r1, gs, ge;
};

__device__ __forceinline__ PairView view_pair(const EdArgs& a, uint64_t i) {
    PairView v{};
    const uint32_t p = a.pairs[3 * i], g = a.pairs[3 * i + 1];
    v.e = a.pairs[3 * i + 2];
    if (p >= a.n_pat || g >= a.n_grp) return v;
    const uint64_t p0 = a.pat_off[p], p1 = a.pat_off[p + 1];
    if (p1 > a.pat_bytes || p0 >= p1 || p1 - p0 > kMaxPattern) return v;
    const uint64_t r0 = a.grp[g], r1 = a.grp[g + 1];
    if (r0 > r1 || r1 > a.n_rec) return v;
    const uint64_t gs = a.rec[r0], ge = a.rec[r1];
    if (gs > ge || ge > a.text_bytes) return v;
    v.ok = true;
    v.m = (uint32_t)(p1 - p0);
    v.p0 = p0, v.r0 = r0, v.r1 = r1, v.gs = gs, v.ge = ge;
    return v;
}

__device__ __forceinline__ uint32_t words_of(uint32_t m) { return m <= 64 ? 1u : m <= 128 ? 2u : m <= 256 ? 4u : 8u; }

__global__ __launch_bounds__(256) void edit_plan_kernel(EdArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) a.pref[0] = 0;
    if (i >= a.n_pairs) return;
    const PairView v = view_pair(a, i);
    uint64_t units = 0, key = kBadPair;
    if (v.ok) {
        const uint64_t per_unit = 64ull * a.chunk;
        units = (v.ge - v.gs + per_unit - 1) / per_unit;
        // end 0 of the group's first record: distance m, the lowest position there is
        key = v.r1 > v.r0 && v.m <= v.e ? (uint64_t)v.m << kPosBits : kNoKey;
    }
    a.pref[i + 1] = units;
    a.keys[i] = key;
}

// the pair that owns unit u: the first i with pref[i + 1] > u (u < pref[n])
__device__ __forceinline__ uint64_t pair_of_unit(const uint64_t* pref, uint64_t n, uint64_t u) {
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pref[mid + 1] > u) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the record of [r0, r1) that holds byte x (rec[r0] <= x < rec[r1]): the last r with rec[r] <= x
__device__ __forceinline__ uint64_t record_of(const uint64_t* rec, uint64_t r0, uint64_t r1, uint64_t x) {
    uint64_t lo = r0 + 1, hi = r1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rec[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
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
    const uintptr_t text_lo = (uintptr_t)a.text, text_hi = text_lo + a.text_bytes;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t pair = pair_of_unit(a.pref, a.n_pairs, u);
        const PairView v = view_pair(a, pair);
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
        const uint64_t ca = v.gs + (slice * 64 + lane) * (uint64_t)a.chunk;
        const uint64_t cb = ca + a.chunk < v.ge ? ca + a.chunk : v.ge;
        uint64_t best = kNoKey;
        if (ca < v.ge) {
            uint64_t r = record_of(a.rec, v.r0, v.r1, ca);
            uint64_t rs = a.rec[r], re = a.rec[r + 1];
            // (offsets that do not ascend cannot take a load outside [gs, ge): every byte index below stays in [start, cb))
            if (rs < v.gs || rs > ca) rs = ca;
            const uint64_t start = ca - rs > lead ? ca - lead : rs;
            uint64_t pv[W], mv[W];
#pragma unroll
            for (int w = 0; w < W; ++w) pv[w] = ~0ULL, mv[w] = 0;
            uint32_t score = m;
            const uintptr_t first = (text_lo + start) & ~(uintptr_t)15, last = text_lo + cb;
            for (uintptr_t blk = first; blk < last; blk += 16) {
                ed4 raw;
                if (blk >= text_lo && blk + 16 <= text_hi) raw = *reinterpret_cast<const ed4*>(blk);
                else {
                    uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int b = 0; b < 16; ++b)
                        if (blk + b >= text_lo && blk + b < text_hi) q[b >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(blk + b) << (8 * (b & 3));
                    raw = ed4{q[0], q[1], q[2], q[3]};
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t word = q == 0 ? raw.x : q == 1 ? raw.y : q == 2 ? raw.z : raw.w;
#pragma nounroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        // The byte's index in the text.  Where the block begins below text_lo (the buffer is not 16-byte
                        // aligned), blk - text_lo is -k in unsigned arithmetic, k = 1..15: the bytes below text_lo get an index
                        // of 2^64 - k + offset >= cb and are skipped, the bytes at and above it wrap back to their true index
                        // offset - k.  The record-boundary handling below relies on t being exact there.
                        const uint64_t t = (uint64_t)(blk - text_lo) + 4u * q + b;
                        if (t < start || t >= cb) continue;
                        if (t >= re) {  // the record ended: a fresh state in the next one that has bytes
                            do {
                                ++r;
                                re = r + 1 <= v.r1 ? a.rec[r + 1] : v.ge;
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

__global__ __launch_bounds__(256) void edit_finish_kernel(EdArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_pairs) return;
    const uint64_t key = a.keys[i];
    uint32_t d = 0xFFFFFFFFu, r = 0xFFFFFFFFu, j = 0xFFFFFFFFu;
    if (key == kBadPair) r = j = 0xFFFFFFFEu;
    else if (key != kNoKey) {
        const PairView v = view_pair(a, i);
        const uint64_t pos = key & ((1ULL << kPosBits) - 1);
        // the last record of the group whose end 0 is at or before pos: position of (r, 0) = rec[r] - gs + (r - r0)
        uint64_t lo = v.r0 + 1, hi = v.r1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (a.rec[mid] - v.gs + (mid - v.r0) > pos) hi = mid;
            else lo = mid + 1;
        }
        const uint64_t rr = lo - 1;
        d = (uint32_t)(key >> kPosBits);
        r = (uint32_t)rr;
        j = (uint32_t)(pos - (a.rec[rr] - v.gs + (rr - v.r0)));
    }
    a.out[3 * i] = d;
    a.out[3 * i + 1] = r;
    a.out[3 * i + 2] = j;
}

uint32_t chunk_knob() {
    const char* e = std::getenv("TXQ_EDIT_CHUNK");
    long long c = e && *e ? std::atoll(e) : (long long)kDefaultChunk;
    if (c < (long long)kMinChunk) c = kMinChunk;
    if (c > (long long)kMaxChunk) c = kMaxChunk;
    return (uint32_t)((c + 15) / 16 * 16);
}

int edit_args(const void* pat_off, const void* rec, const void* grp, const void* pairs, size_t n_pairs, size_t n_records, size_t text_bytes,
              const void* codes, const void* out) {
    if (!pat_off || !rec || !grp || !codes || (n_pairs && (!pairs || !out))) return fail(TXQ_ERR_ARG, "null argument");
    if (n_pairs > 0x7FFFFFFFull || n_records >= 0xFFFFFFFEull) return fail(TXQ_ERR_ARG, "at most 2^31 pairs and 2^32 - 2 records per call");
    if ((uint64_t)text_bytes + n_records >= 1ULL << kPosBits) return fail(TXQ_ERR_ARG, "text too large for one call");
    return TXQ_OK;
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

int txq_edit_search_device(const uint8_t* d_patterns, const uint64_t* d_pat_offsets, size_t n_patterns, size_t pattern_bytes,
                           const uint8_t* d_text, const uint64_t* d_rec_offsets, size_t n_records, size_t text_bytes,
                           const uint64_t* d_group_offsets, size_t n_groups, const uint32_t* d_pairs, size_t n_pairs,
                           const uint8_t* d_codes, uint32_t* d_out, void* d_workspace, void* stream) {
    if (int rc = edit_args(d_pat_offsets, d_rec_offsets, d_group_offsets, d_pairs, n_pairs, n_records, text_bytes, d_codes, d_out)) return rc;
    if (n_pairs && (!d_workspace || ((uintptr_t)d_workspace & 7))) return fail(TXQ_ERR_ARG, "the workspace must be an 8-byte aligned device pointer");
    if ((pattern_bytes && !d_patterns) || (text_bytes && !d_text)) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) return TXQ_OK;
    hipStream_t st = (hipStream_t)stream;
    void* scratch = d_workspace;  // keys and prefix: TXQ_EDIT_WORKSPACE(n_pairs) bytes of the caller's
    const EdArgs a{d_patterns, d_pat_offsets, n_patterns, pattern_bytes, d_text, d_rec_offsets, n_records, text_bytes, d_group_offsets, n_groups,
                   d_pairs, n_pairs, d_codes, d_out, (uint64_t*)scratch, (uint64_t*)scratch + n_pairs, chunk_knob()};
    const unsigned per_pair = (unsigned)((n_pairs + 255) / 256);
    edit_plan_kernel<<<per_pair, 256, 0, st>>>(a);
    scan_kernel<<<1, 1024, 0, st>>>(a.pref + 1, n_pairs);
    edit_kernel<1><<<kGridBlocks, 64, 0, st>>>(a);
    edit_kernel<2><<<kGridBlocks, 64, 0, st>>>(a);
    edit_kernel<4><<<kGridBlocks, 64, 0, st>>>(a);
    edit_kernel<8><<<kGridBlocks, 64, 0, st>>>(a);
    edit_finish_kernel<<<per_pair, 256, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "edit kernel launch");
    return TXQ_OK;
}

int txq_edit_search(const uint8_t* patterns, const uint64_t* pat_offsets, size_t n_patterns, const uint8_t* text, const uint64_t* rec_offsets,
                    size_t n_records, const uint64_t* group_offsets, size_t n_groups, const uint32_t* pairs, size_t n_pairs,
                    const uint8_t* codes, uint32_t* out) {
    if (!pat_offsets || !rec_offsets || !group_offsets) return fail(TXQ_ERR_ARG, "null argument");
    for (size_t p = 0; p < n_patterns; ++p)
        if (pat_offsets[p + 1] < pat_offsets[p]) return fail(TXQ_ERR_ARG, "pattern offsets are not ascending at pattern %zu", p);
    for (size_t r = 0; r < n_records; ++r)
        if (rec_offsets[r + 1] < rec_offsets[r]) return fail(TXQ_ERR_ARG, "record offsets are not ascending at record %zu", r);
    for (size_t g = 0; g < n_groups; ++g)
        if (group_offsets[g + 1] < group_offsets[g] || group_offsets[g + 1] > n_records)
            return fail(TXQ_ERR_ARG, "group offsets are not ascending within the records at group %zu", g);
    const uint64_t pat0 = pat_offsets[0], pat_bytes = pat_offsets[n_patterns] - pat0;
    const uint64_t text0 = rec_offsets[0], text_bytes = rec_offsets[n_records] - text0;
    if (int rc = edit_args(pat_offsets, rec_offsets, group_offsets, pairs, n_pairs, n_records, text_bytes, codes, out)) return rc;
    if ((pat_bytes && !patterns) || (text_bytes && !text)) return fail(TXQ_ERR_ARG, "null argument");
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t p = pairs[3 * i], g = pairs[3 * i + 1];
        if (p >= n_patterns || g >= n_groups) return fail(TXQ_ERR_ARG, "pair %zu names pattern %u of %zu, group %u of %zu", i, p, n_patterns, g, n_groups);
        const uint64_t m = pat_offsets[p + 1] - pat_offsets[p];
        if (m < 1 || m > kMaxPattern) return fail(TXQ_ERR_ARG, "pair %zu: a pattern of %llu bytes (1..%u run on the device)", i, (unsigned long long)m, kMaxPattern);
    }
    if (int rc = require_init()) return rc;
    if (n_pairs == 0) return TXQ_OK;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_pat = up(pat_bytes + 16), b_po = up((n_patterns + 1) * 8), b_text = up(text_bytes + 16), b_rec = up((n_records + 1) * 8),
                 b_grp = up((n_groups + 1) * 8), b_pairs = up(n_pairs * 12), b_codes = 256, b_out = up(n_pairs * 12), b_work = up(TXQ_EDIT_WORKSPACE(n_pairs));
    unsigned char* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, b_pat + b_po + b_text + b_rec + b_grp + b_pairs + b_codes + b_out + b_work);
    if (e != hipSuccess) return fail_hip(e, "hipMalloc");
    unsigned char* at = d;
    auto take = [&](size_t b) { unsigned char* p = at; at += b; return p; };
    uint8_t* d_pat = take(b_pat);
    uint64_t* d_po = (uint64_t*)take(b_po);
    uint8_t* d_text = take(b_text);
    uint64_t* d_rec = (uint64_t*)take(b_rec);
    uint64_t* d_grp = (uint64_t*)take(b_grp);
    uint32_t* d_pairs = (uint32_t*)take(b_pairs);
    uint8_t* d_codes = take(b_codes);
    uint32_t* d_out = (uint32_t*)take(b_out);
    void* d_work = take(b_work);
    std::vector<uint64_t> po(pat_offsets, pat_offsets + n_patterns + 1), ro(rec_offsets, rec_offsets + n_records + 1);
    for (uint64_t& o : po) o -= pat0;
    for (uint64_t& o : ro) o -= text0;
    int rc = TXQ_OK;
    if (pat_bytes) e = hipMemcpy(d_pat, patterns + pat0, pat_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_po, po.data(), po.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && text_bytes) e = hipMemcpy(d_text, text + text0, text_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rec, ro.data(), ro.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_grp, group_offsets, (n_groups + 1) * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_pairs, pairs, n_pairs * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_codes, codes, 256, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        rc = txq_edit_search_device(d_pat, d_po, n_patterns, pat_bytes, d_text, d_rec, n_records, text_bytes, d_grp, n_groups, d_pairs, n_pairs,
                                    d_codes, d_out, d_work, nullptr);
    if (e == hipSuccess && rc == TXQ_OK) e = hipMemcpy(out, d_out, n_pairs * 12, hipMemcpyDeviceToHost);  // (waits for the kernels)
    (void)hipFree(d);
    if (e != hipSuccess) return fail_hip(e, "txq_edit_search copies");
    return rc;
}

}  // extern "C"
