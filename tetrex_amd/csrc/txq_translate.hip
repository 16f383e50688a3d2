// Six-frame translation of nucleotide records into the k-mer values of a peptide index, and the compact list of a hit
// matrix, on gfx950 (txq_translate / txq_translate_device, txq_hit_list_device; `tetrex search --translate`).
// The reference has no counterpart: it never asks an index about a sequence.
//
// Translation.  Record r is seq[rec[r] .. rec[r+1]), L bytes.  The window S[p, p + 3k) of the record is at once
//   * the forward k-mer at codon p / 3 of frame +(p mod 3 + 1), and
//   * reverse-complemented, the k-mer at codon (L - p - 3k) / 3 of frame -((L - p - 3k) mod 3 + 1),
// so one pass over the start positions p serves all six frames.  A k-mer is a value when none of its k residues is a stop;
// query 6 r + f owns the values of frame f in ascending codon order, which for a forward frame is ascending p and for a
// reverse frame descending p.  This is stream compaction: count, scan, fill.
//
// Mapping to the machine:
//   * the bytes rec[0] .. rec[n] are cut into at most kUnits units of `chunk` start positions (a multiple of kTile, known
//     only on the device: no host synchronisation), one wave each, so a record of 2 x 10^6 bytes is spread over thousands
//     of waves and a unit of short reads walks the records that start in it;
//   * a step takes kTile = 192 start positions of one record, aligned to the record's codons: lane l owns p = t0 + 3 l + j,
//     j = 0, 1, 2, so j is the forward frame.  The step's bytes are staged with 16-byte loads into LDS, every codon is
//     translated once in both directions into the index's residue codes (LDS), and a lane folds the k codes of each of
//     its windows;
//   * the rank of a value inside its frame is (valid windows of the frame before this step) + (valid lanes below, from one
//     ballot per frame and direction): consecutive lanes write consecutive 8-byte values, a 512-byte store per wave;
//   * count_kernel adds each record's six counts into offsets[] and leaves, per unit, the counts of the record that runs
//     past the unit's end; scan_kernel turns the counts into offsets; fill_kernel recomputes the windows and, for a record
//     that began in an earlier unit, first sums those units' counts.
// Scratch (6 u32 per unit; the hit list's tile sums) is allocated and freed in stream order by the library.
// The same pass with the frames as residue letters instead of values (txq_translate_frames*) is frames_kernel below.
// The fill pass that also cuts every frame into windows and writes each window's range of values (txq_translate_windows*,
// DESIGN.md §18) is translate_windows_kernel: the same body, instantiated with a compile-time flag.
#include "../../include/txq.h"
#include "txq_internal.hpp"
#include "txq_frames_plan.hpp"
#include "txq_frame_windows_plan.hpp"
#include "txq_scan.hpp"

namespace txq {
namespace {

using namespace tr;                         // kUnits, kTile, chunk_len, nucleotide and the frames' addresses: txq_frames_plan.hpp
constexpr uint32_t kMaxK = 12;               // 5 bits per residue in 64 (and the staging buffers below)
constexpr uint32_t kRawBytes = 256;          // 15 (alignment) + kTile + 3 kMaxK - 1 = 242 bytes at most
constexpr uint32_t kResidues = 256;          // kTile + 3 (kMaxK - 1) = 225 residues at most
constexpr uint8_t kStop = 0xFF;

// NCBI translation table 1, codon index 16 a + 4 b + c with T = 0, C = 1, A = 2, G = 3
__constant__ char kTable1[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

struct TrArgs {
    const uint8_t* seq;
    const uint64_t* rec;  // n + 1
    uint64_t n;
    uint32_t k;
    const uint8_t* codes;  // 256
    uint64_t* values;
    uint64_t* offsets;  // 6 n + 1
    uint32_t* tails;    // kUnits x 6: per unit, the counts (forward j, reverse j) of the record that runs past the unit's end
};

// what the fill pass writes besides the values when it also cuts the frames into windows (translate_windows_kernel below)
struct WinArgs {
    uint32_t window, step;        // residues
    const uint64_t* win_offsets;  // 6 n + 1, complete
    uint64_t* begin;              // per window: V(begin boundary), relative to the frame's first value
    uint32_t* end;                // per window: the low 32 bits of V(end boundary), likewise
};

template <bool FILL, bool WIN>
__device__ __forceinline__ void translate_pass(const TrArgs& a, const WinArgs& w) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[kRawBytes];
    __shared__ uint8_t res[2][kResidues];  // residue codes of the codon at t0 + i: forward, reverse-complemented
    __shared__ uint8_t lut[64];            // codon -> residue code of this index, kStop for a stop
    const uint32_t lane = threadIdx.x;
    const uint64_t base = a.rec[0], end = a.rec[a.n];
    if (end <= base) return;
    const uint64_t chunk = chunk_len(end - base);
    const uint64_t ua = base + (uint64_t)blockIdx.x * chunk;
    if (ua >= end) return;
    const uint64_t ub = ua + chunk < end ? ua + chunk : end;
    {
        const char aa = kTable1[lane];
        lut[lane] = aa == '*' ? kStop : (uint8_t)(a.codes[(uint8_t)aa] & 31u);
    }
    const uint8_t code_x = (uint8_t)(a.codes[(uint8_t)'X'] & 31u);
    const uint32_t k = a.k, span = 3u * k;
    const uint64_t below = (1ULL << lane) - 1ULL;
    const uintptr_t seq_lo = (uintptr_t)(a.seq + base), seq_hi = (uintptr_t)(a.seq + end);
    __syncthreads();

    uint32_t cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // (count) windows of the current record in this unit: forward j, reverse j
    bool runs_on = false;                        // the current record runs past the unit's end
    for (uint64_t r = record_of(a.rec, 0, a.n, ua); r < a.n; ++r) {
        const uint64_t rs = a.rec[r];
        if (rs >= ub) break;
        const uint64_t re = a.rec[r + 1], L = re - rs;
#pragma unroll
        for (int c = 0; c < 6; ++c) cnt[c] = 0u;
        runs_on = re > ub;
        if (L < span) continue;
        const uint64_t lo = (ua > rs ? ua : rs) - rs;                         // start positions [lo, hi) of this record are this unit's
        const uint64_t fit = L - span + 1, cut = (ub < re ? ub : re) - rs;
        const uint64_t hi = cut < fit ? cut : fit;
        if (lo >= hi) continue;
        // frame of the reverse windows at p = j (mod 3), and where the frames' values go
        uint32_t rframe[3];
        uint64_t fbase[3], rlast[3], run[6];
        fw::Frame wplan[6];            // (WIN) the windows of forward frame j, of the reverse frame of p = j (mod 3)
        uint64_t wbase[6], rcount[3];  // (WIN) their first window slots; the value count of that reverse frame
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            rframe[j] = 3u + (uint32_t)((L - span + 3u - (uint32_t)j) % 3u);  // (L - 3k - p) mod 3 for every p = j (mod 3) that fits
            run[j] = run[3 + j] = 0;
            if (FILL) {
                fbase[j] = a.offsets[6 * r + j];
                rlast[j] = a.offsets[6 * r + rframe[j] + 1] - 1;  // the frame's first codon is its last start position
            }
            if (WIN) {
                wplan[j] = fw::frame_plan(frame_len(L, (uint32_t)j), k, w.window, w.step);
                wplan[3 + j] = fw::frame_plan(frame_len(L, rframe[j] - 3u), k, w.window, w.step);
                wbase[j] = w.win_offsets[6 * r + j];
                wbase[3 + j] = w.win_offsets[6 * r + rframe[j]];
                rcount[j] = a.offsets[6 * r + rframe[j] + 1] - a.offsets[6 * r + rframe[j]];
            }
        }
        if (FILL && lo > 0) {  // the record began in an earlier unit: the windows those units found
            const uint64_t u0 = (rs - base) / chunk;
            uint64_t part[6] = {0, 0, 0, 0, 0, 0};
            for (uint64_t u = u0 + lane; u < blockIdx.x; u += 64)
#pragma unroll
                for (int c = 0; c < 6; ++c) part[c] += a.tails[u * 6 + c];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                uint64_t v = part[c];
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
                run[c] = v;
            }
        }
        for (uint64_t t0 = lo / 3 * 3; t0 < hi; t0 += kTile) {
            // stage the step's bytes: 16-byte blocks, 'N' for what lies outside the sequence buffer (txq_text.hpp load_block)
            const uintptr_t first = (uintptr_t)(a.seq + rs + t0);
            const uint32_t shift = (uint32_t)(first & 15u);
            const uint64_t left = L - t0;
            const uint32_t nbytes = left < kTile + span - 1 ? (uint32_t)left : kTile + span - 1;
            if (lane < (shift + nbytes + 15u) / 16u)
                *reinterpret_cast<text4*>(raw + 16u * lane) = load_block(first - shift + 16u * lane, seq_lo, seq_hi, 'N').w;
            __syncthreads();
            for (uint32_t i = lane; i < kTile + span - 3; i += 64) {
                uint8_t f = kStop, g = kStop;  // (a codon that does not fit is never part of a window that fits)
                if (t0 + i + 3 <= L) {
                    const uint32_t x = nucleotide(raw[shift + i]), y = nucleotide(raw[shift + i + 1]), z = nucleotide(raw[shift + i + 2]);
                    if ((x | y | z) & 4u) f = g = code_x;
                    else {
                        f = lut[16u * x + 4u * y + z];
                        g = lut[16u * (z ^ 2u) + 4u * (y ^ 2u) + (x ^ 2u)];
                    }
                }
                res[0][i] = f;
                res[1][i] = g;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint64_t p = t0 + 3u * lane + (uint32_t)j;
                const bool mine = p >= lo && p < hi;
                uint64_t vf = 0, vr = 0;
                bool okf = mine, okr = mine;
                if (mine) {
                    const uint32_t at = 3u * lane + (uint32_t)j;
                    for (uint32_t q = 0; q < k; ++q) {
                        const uint8_t f = res[0][at + 3u * q], g = res[1][at + 3u * q];
                        okf = okf && f != kStop;
                        okr = okr && g != kStop;
                        vf = (vf << 5) | (uint64_t)(f & 31u);
                        vr |= (uint64_t)(g & 31u) << (5u * q);  // the window's last codon is the reverse k-mer's first residue
                    }
                }
                const uint64_t bf = __ballot(okf), br = __ballot(okr);
                if (WIN && mine) {
                    // V at this lane's k-mer position in either frame: the rank its value is (or would be) written at, and
                    // the same counted from the frame's far end.  Each window slot has one owner (txq_frame_windows_plan.hpp).
                    const uint64_t vfw = run[j] + (uint64_t)__builtin_popcountll(bf & below);
                    const fw::Slots sf = fw::codon_slots(wplan[j], p / 3);
                    if (sf.begin != fw::kNone) w.begin[wbase[j] + sf.begin] = vfw;
                    if (sf.end != fw::kNone) w.end[wbase[j] + sf.end] = (uint32_t)vfw;
                    const uint64_t vrv = rcount[j] - (run[3 + j] + (uint64_t)__builtin_popcountll(br & below) + (okr ? 1u : 0u));
                    const fw::Slots sr = fw::codon_slots(wplan[3 + j], fw::rev_kmer_index(L, p, k));
                    if (sr.begin != fw::kNone) w.begin[wbase[3 + j] + sr.begin] = vrv;
                    if (sr.end != fw::kNone) w.end[wbase[3 + j] + sr.end] = (uint32_t)vrv;
                }
                if (FILL) {
                    if (okf) a.values[fbase[j] + run[j] + (uint64_t)__builtin_popcountll(bf & below)] = vf;
                    if (okr) a.values[rlast[j] - run[3 + j] - (uint64_t)__builtin_popcountll(br & below)] = vr;
                    run[j] += (uint64_t)__builtin_popcountll(bf);
                    run[3 + j] += (uint64_t)__builtin_popcountll(br);
                } else {
                    cnt[j] += (uint32_t)__builtin_popcountll(bf);
                    cnt[3 + j] += (uint32_t)__builtin_popcountll(br);
                }
            }
            __syncthreads();
        }
        if (!FILL && lane == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (cnt[j]) atomicAdd((unsigned long long*)(a.offsets + 1 + 6 * r + j), (unsigned long long)cnt[j]);
                if (cnt[3 + j]) atomicAdd((unsigned long long*)(a.offsets + 1 + 6 * r + rframe[j]), (unsigned long long)cnt[3 + j]);
            }
        }
    }
    if (!FILL && lane < 6) {
        uint32_t mine = 0;
#pragma unroll
        for (int c = 0; c < 6; ++c)
            if (lane == (uint32_t)c) mine = cnt[c];
        a.tails[(uint64_t)blockIdx.x * 6 + lane] = runs_on ? mine : 0u;
    }
}

template <bool FILL>
__global__ __launch_bounds__(64) void translate_kernel(TrArgs a) {
    translate_pass<FILL, false>(a, WinArgs{});
}

// ---- windows of the frames ------------------------------------------------------------------------------------------------
// txq_translate_windows_device: the fill pass once more, and while a lane holds the rank of its k-mer position
// it stores that rank into the window slots the position bounds.  The number of windows of a frame is closed-form in L
// (window_counts_kernel, then scan_kernel); a window's begin and end may be written by different waves, so the pass writes
// them relative to the frame and window_finish_kernel turns them into (first value, value count) afterwards.
__global__ __launch_bounds__(64) void translate_windows_kernel(TrArgs a, WinArgs w) {
    translate_pass<true, true>(a, w);
}

__global__ __launch_bounds__(256) void window_counts_kernel(const uint64_t* __restrict__ rec, uint64_t n, uint32_t k, uint32_t window, uint32_t step,
                                                            uint64_t* __restrict__ win_offsets) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) win_offsets[0] = 0;
    if (r >= n) return;
    const uint64_t L = rec[r + 1] - rec[r];
#pragma unroll
    for (uint32_t f = 0; f < 6; ++f) win_offsets[1 + 6 * r + f] = fw::window_count(frame_len(L, f % 3), k, window, step);
}

constexpr uint32_t kFinishBlocks = 1024;
// window j of frame q: begin[j] = offsets[q] + V(begin boundary), len[j] = V(end boundary) - V(begin boundary); the end
// boundary of the frame's last window is the frame's end, which no start position owns: V there is the frame's value count
__global__ __launch_bounds__(256) void window_finish_kernel(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ win_offsets, uint64_t m,
                                                            uint64_t* __restrict__ begin, uint32_t* __restrict__ len) {
    const uint64_t total = win_offsets[m];
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (uint64_t)kFinishBlocks * 256) {
        uint64_t lo = 0, hi = m;  // the frame q with win_offsets[q] <= j < win_offsets[q + 1]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (win_offsets[mid] <= j) lo = mid;
            else hi = mid;
        }
        const uint64_t b = begin[j];
        const uint32_t e = j + 1 == win_offsets[lo + 1] ? (uint32_t)(offsets[lo + 1] - offsets[lo]) : len[j];
        begin[j] = offsets[lo] + b;
        len[j] = e - (uint32_t)b;
    }
}

// ---- frames as letters ----------------------------------------------------------------------------------------------------
// txq_translate_frames_device: the six frames of every record as residue letters, back to back, in the form
// the edit-distance kernels take their patterns.  The pass is translate_kernel's — the same units, the same steps of kTile
// start positions, the same staging of the bytes — but nothing is compacted: a frame's length is closed-form in L, so the
// offsets are a per-record fill and a scan, and the codon at start position p has its place in both directions
// (txq_frames_plan.hpp).  A step yields six runs of up to 64 letters, which are staged in LDS at their address modulo 16 and
// stored as the 16-byte blocks, 4-byte words and single bytes that lie inside the run (store_block): the units next to this
// one write the bytes next to the run, so no store covers a byte that is not the run's and nothing is read back.

struct FrArgs {
    const uint8_t* seq;
    const uint64_t* rec;  // n + 1
    uint64_t n;
    uint8_t* frames;
    uint64_t cap;             // bytes of `frames`: nothing at or behind it is written
    const uint64_t* offsets;  // 6 n + 1, complete
};

__global__ __launch_bounds__(256) void frame_lengths_kernel(const uint64_t* __restrict__ rec, uint64_t n, uint64_t* __restrict__ offsets) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) offsets[0] = 0;
    if (r >= n) return;
    const uint64_t L = rec[r + 1] - rec[r];
#pragma unroll
    for (uint32_t f = 0; f < 6; ++f) offsets[1 + 6 * r + f] = frame_len(L, f % 3);
}

struct GlobalSink {
    __device__ __forceinline__ void store16(uintptr_t at, const uint8_t* src) { *reinterpret_cast<text4*>(at) = *reinterpret_cast<const text4*>(src); }
    __device__ __forceinline__ void store4(uintptr_t at, const uint8_t* src) { *reinterpret_cast<uint32_t*>(at) = *reinterpret_cast<const uint32_t*>(src); }
    __device__ __forceinline__ void store1(uintptr_t at, uint8_t byte) { *reinterpret_cast<uint8_t*>(at) = byte; }
};

__global__ __launch_bounds__(64) void frames_kernel(FrArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[kRawBytes];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kRuns][kStageRow];  // run c, the byte for address x at x - block_floor(run_a0[c])
    __shared__ uint64_t run_org[kRuns], run_a0[kRuns], run_a1[kRuns];         // the run's frame begins at org; the run is the addresses [a0, a1)
    const uint32_t lane = threadIdx.x;
    const uint64_t base = a.rec[0], end = a.rec[a.n];
    if (end <= base) return;
    const uint64_t chunk = chunk_len(end - base);
    const uint64_t ua = base + (uint64_t)blockIdx.x * chunk;
    if (ua >= end) return;
    const uint64_t ub = ua + chunk < end ? ua + chunk : end;
    const uintptr_t seq_lo = (uintptr_t)(a.seq + base), seq_hi = (uintptr_t)(a.seq + end);
    const uintptr_t out_lo = (uintptr_t)a.frames, out_hi = out_lo + a.cap;
    GlobalSink sink;
    for (uint64_t r = record_of(a.rec, 0, a.n, ua); r < a.n; ++r) {
        const uint64_t rs = a.rec[r];
        if (rs >= ub) break;
        const uint64_t re = a.rec[r + 1], L = re - rs;
        if (L < 3) continue;
        const Owned own = owned_starts(rs, re, ua, ub);
        if (own.lo >= own.hi) continue;
        uint64_t org = 0;
        if (lane < kRuns) run_org[lane] = org = out_lo + a.offsets[6 * r + run_frame(L, lane)];
        for (uint64_t t0 = own.lo / 3 * 3; t0 < own.hi; t0 += kTile) {
            // stage the step's bytes: 16-byte blocks, 'N' for what lies outside the sequence buffer (txq_text.hpp load_block)
            const uintptr_t first = (uintptr_t)(a.seq + rs + t0);
            const uint32_t shift = (uint32_t)(first & 15u);
            const uint64_t left = L - t0;
            const uint32_t nbytes = left < kTile + 2 ? (uint32_t)left : kTile + 2;
            if (lane < (shift + nbytes + 15u) / 16u)
                *reinterpret_cast<text4*>(raw + 16u * lane) = load_block(first - shift + 16u * lane, seq_lo, seq_hi, 'N').w;
            if (lane < kRuns) {
                const Run q = step_run(L, t0, own, lane);
                run_a0[lane] = org + q.first;
                run_a1[lane] = org + q.first + q.count;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t i = lane; i < kTile; i += 64) {
                const uint64_t p = t0 + i;
                if (p < own.lo || p >= own.hi) continue;  // (hi <= L - 2: the codon fits)
                const uint32_t j = i % 3;                 // = p mod 3
                uint8_t f, g;
                codon_letters(kTable1, nucleotide(raw[shift + i]), nucleotide(raw[shift + i + 1]), nucleotide(raw[shift + i + 2]), &f, &g);
                stage[j][run_org[j] + fwd_index(p) - block_floor(run_a0[j])] = f;
                stage[3 + j][run_org[3 + j] + rev_index(L, p) - block_floor(run_a0[3 + j])] = g;
            }
            __syncthreads();
            if (lane < kRuns * kRunBlocks) {
                const uint32_t c = lane / kRunBlocks, b = lane % kRunBlocks;
                const uintptr_t a0 = run_a0[c], a1 = run_a1[c] < out_hi ? run_a1[c] : out_hi;
                const uintptr_t blk = block_floor(a0) + 16u * b;
                const uint32_t mask = block_mask(a0, a1, blk);
                if (mask) store_block(mask, blk, &stage[c][16u * b], sink);
            }
            __syncthreads();
        }
    }
}

// ---- hit list -----------------------------------------------------------------------------------------------------------
// Tiles of kHitTile words of the hit matrix, 4 consecutive words per thread: the tiles' bit counts, their scan (scan_kernel),
// then every thread writes the triples of its words from its rank.  The order is (word index, bit) = (query, bin).

constexpr uint32_t kHitThreads = 256, kHitTile = 4 * kHitThreads;

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kHitThreads / 64; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(kHitThreads) void hit_count_kernel(const uint64_t* __restrict__ hits, uint64_t m, uint64_t* tile_pref) {
    __shared__ uint32_t wsum[kHitThreads / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kHitTile + threadIdx.x * 4u;
    uint32_t c = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i0 + e < m) c += (uint32_t)__builtin_popcountll(hits[i0 + e]);
    uint32_t total;
    (void)block_exclusive_scan(c, wsum, &total);
    if (threadIdx.x == 0) {
        tile_pref[(uint64_t)blockIdx.x + 1] = total;
        if (blockIdx.x == 0) tile_pref[0] = 0;
    }
}

__global__ __launch_bounds__(kHitThreads) void hit_fill_kernel(const uint64_t* __restrict__ hits, const uint32_t* __restrict__ counts, uint64_t m,
                                                               uint64_t words, const uint64_t* __restrict__ tile_pref, uint64_t n_tiles,
                                                               uint32_t* __restrict__ list, uint64_t capacity, uint64_t* total_out) {
    __shared__ uint32_t wsum[kHitThreads / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kHitTile + threadIdx.x * 4u;
    uint64_t w[4];
    uint32_t c = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        w[e] = i0 + e < m ? hits[i0 + e] : 0;
        c += (uint32_t)__builtin_popcountll(w[e]);
    }
    uint32_t total;
    uint64_t at = tile_pref[blockIdx.x] + block_exclusive_scan(c, wsum, &total);
    if (blockIdx.x == 0 && threadIdx.x == 0) *total_out = tile_pref[n_tiles];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint64_t bits = w[e];
        if (!bits) continue;
        const uint64_t q = (i0 + e) / words, word = (i0 + e) % words;
        while (bits && at < capacity) {
            const uint32_t bin = (uint32_t)(word * 64) + (uint32_t)__builtin_ctzll(bits);
            bits &= bits - 1;
            list[3 * at] = (uint32_t)q;
            list[3 * at + 1] = bin;
            list[3 * at + 2] = counts ? counts[q * words * 64 + bin] : 0u;
            ++at;
        }
        at += (uint64_t)__builtin_popcountll(bits);  // (what did not fit still counts towards the ranks that follow)
    }
}

int translate_args(const void* seq, const void* rec, size_t n, unsigned k, const void* codes, const void* values, const void* offsets) {
    if (k < 1 || k > kMaxK) return fail(TXQ_ERR_ARG, "k = %u: translated k-mers need k in 1..12", k);
    if (!offsets || (n && (!rec || !codes))) return fail(TXQ_ERR_ARG, "null argument");
    (void)seq; (void)values;  // (may be null where there are no bytes / no values: only the caller knows)
    if (n > 0x7FFFFFFFull / 6) return fail(TXQ_ERR_ARG, "at most 2^31 / 6 records per call");
    return TXQ_OK;
}

}  // namespace
}  // namespace txq

using namespace txq;

extern "C" {

uint64_t txq_translate_bound(const uint64_t* rec_offsets, size_t n_records, unsigned k) {
    if (k < 1 || k > kMaxK || (n_records && !rec_offsets)) {
        (void)fail(TXQ_ERR_ARG, "txq_translate_bound: null offsets or k outside 1..12");
        return UINT64_MAX;
    }
    if (check_ascending(rec_offsets, n_records, "record")) return UINT64_MAX;
    uint64_t bound = 0;
    for (size_t r = 0; r < n_records; ++r) {
        const uint64_t L = rec_offsets[r + 1] - rec_offsets[r];
        for (uint64_t o = 0; o < 3; ++o) {
            const uint64_t codons = L >= o ? (L - o) / 3 : 0;
            if (codons >= k) bound += 2 * (codons - k + 1);
        }
    }
    return bound;
}

int txq_translate_device(const uint8_t* d_seq, const uint64_t* d_rec_offsets, size_t n_records, unsigned k, const uint8_t* d_codes,
                         uint64_t* d_values, uint64_t* d_offsets, void* stream) {
    if (int rc = translate_args(d_seq, d_rec_offsets, n_records, k, d_codes, d_values, d_offsets)) return rc;
    if (int rc = require_init()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t m = 6 * n_records;
    hipError_t e = hipMemsetAsync(d_offsets, 0, (m + 1) * 8, st);
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync");
    if (n_records == 0) return TXQ_OK;
    void* tails = nullptr;
    if (e = hipMallocAsync(&tails, (size_t)kUnits * 6 * 4, st); e != hipSuccess) return fail_hip(e, "hipMallocAsync");
    const TrArgs a{d_seq, d_rec_offsets, (uint64_t)n_records, k, d_codes, d_values, d_offsets, (uint32_t*)tails};
    translate_kernel<false><<<kUnits, 64, 0, st>>>(a);
    scan_kernel<<<1, 1024, 0, st>>>(d_offsets + 1, m);
    translate_kernel<true><<<kUnits, 64, 0, st>>>(a);
    e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(tails, st);
    if (e != hipSuccess) return fail_hip(e, "translate kernel launch");
    if (ef != hipSuccess) return fail_hip(ef, "hipFreeAsync");
    return TXQ_OK;
}

int txq_translate(const uint8_t* seq, const uint64_t* rec_offsets, size_t n_records, unsigned k, const uint8_t* codes, uint64_t* values,
                  uint64_t* offsets) {
    if (int rc = translate_args(seq, rec_offsets, n_records, k, codes, values, offsets)) return rc;
    const uint64_t bound = txq_translate_bound(rec_offsets, n_records, k);
    if (bound == UINT64_MAX) return TXQ_ERR_ARG;
    const uint64_t first = n_records ? rec_offsets[0] : 0, bytes = n_records ? rec_offsets[n_records] - first : 0;
    if ((bytes && !seq) || (bound && !values)) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = require_init()) return rc;
    const size_t m = 6 * n_records;
    DeviceStage d;  // (+16: the kernels' 16-byte loads of the sequence end inside the slice; +8: no slice of no bytes)
    const size_t s_seq = d.add(bytes + 16), s_rec = d.add((n_records + 1) * 8), s_codes = d.add(256), s_off = d.add((m + 1) * 8), s_val = d.add(bound * 8 + 8);
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> ro = rebased(rec_offsets, n_records);
    d.upload(s_seq, seq + first, bytes);
    d.upload(s_rec, ro.data(), ro.size() * 8);
    d.upload(s_codes, codes, n_records ? 256 : 0);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_translate_device(d.at<uint8_t>(s_seq), d.at<uint64_t>(s_rec), n_records, k, d.at<uint8_t>(s_codes), d.at<uint64_t>(s_val), d.at<uint64_t>(s_off), nullptr);
    if (rc == TXQ_OK) d.download(offsets, s_off, (m + 1) * 8);  // (waits for the kernels)
    if (rc == TXQ_OK && d.error() == hipSuccess && offsets[m]) {
        if (offsets[m] > bound) rc = fail(TXQ_ERR_OVERFLOW, "translation produced more values than its bound");
        else d.download(values, s_val, offsets[m] * 8);
    }
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_translate copies");
    return rc;
}

uint64_t txq_translate_windows_bound(const uint64_t* rec_offsets, size_t n_records, unsigned k, uint32_t window, uint32_t step) {
    if (k < 1 || k > kMaxK || (n_records && !rec_offsets) || window < k || step < 1 || step > window) {
        (void)fail(TXQ_ERR_ARG, "txq_translate_windows_bound: null offsets, k outside 1..12, window below k or step outside 1..window");
        return UINT64_MAX;
    }
    if (check_ascending(rec_offsets, n_records, "record")) return UINT64_MAX;
    uint64_t bound = 0;
    for (size_t r = 0; r < n_records; ++r)
        for (uint32_t o = 0; o < 3; ++o) bound += 2 * fw::window_count(frame_len(rec_offsets[r + 1] - rec_offsets[r], o), k, window, step);
    return bound;
}

int txq_translate_windows_device(const uint8_t* d_seq, const uint64_t* d_rec_offsets, size_t n_records, unsigned k, const uint8_t* d_codes,
                                 uint32_t window, uint32_t step, uint64_t* d_values, uint64_t* d_offsets, uint64_t* d_win_offsets,
                                 uint64_t* d_win_begin, uint32_t* d_win_len, void* stream) {
    if (int rc = translate_args(d_seq, d_rec_offsets, n_records, k, d_codes, d_values, d_offsets)) return rc;
    if (window < k || step < 1 || step > window) return fail(TXQ_ERR_ARG, "window = %u, step = %u: windows need window >= k and step in 1..window", window, step);
    if (!d_win_offsets || (n_records && (!d_win_begin || !d_win_len))) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = require_init()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t m = 6 * n_records;
    hipError_t e = hipMemsetAsync(d_offsets, 0, (m + 1) * 8, st);
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync");
    if (n_records == 0) {
        e = hipMemsetAsync(d_win_offsets, 0, 8, st);
        return e == hipSuccess ? TXQ_OK : fail_hip(e, "hipMemsetAsync");
    }
    void* tails = nullptr;
    if (e = hipMallocAsync(&tails, (size_t)kUnits * 6 * 4, st); e != hipSuccess) return fail_hip(e, "hipMallocAsync");
    const TrArgs a{d_seq, d_rec_offsets, (uint64_t)n_records, k, d_codes, d_values, d_offsets, (uint32_t*)tails};
    const WinArgs w{window, step, d_win_offsets, d_win_begin, d_win_len};
    translate_kernel<false><<<kUnits, 64, 0, st>>>(a);
    scan_kernel<<<1, 1024, 0, st>>>(d_offsets + 1, m);
    window_counts_kernel<<<(unsigned)((n_records + 255) / 256), 256, 0, st>>>(d_rec_offsets, (uint64_t)n_records, k, window, step, d_win_offsets);
    scan_kernel<<<1, 1024, 0, st>>>(d_win_offsets + 1, m);
    translate_windows_kernel<<<kUnits, 64, 0, st>>>(a, w);
    window_finish_kernel<<<kFinishBlocks, 256, 0, st>>>(d_offsets, d_win_offsets, (uint64_t)m, d_win_begin, d_win_len);
    e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(tails, st);
    if (e != hipSuccess) return fail_hip(e, "translate windows kernel launch");
    if (ef != hipSuccess) return fail_hip(ef, "hipFreeAsync");
    return TXQ_OK;
}

int txq_translate_windows(const uint8_t* seq, const uint64_t* rec_offsets, size_t n_records, unsigned k, const uint8_t* codes, uint32_t window,
                          uint32_t step, uint64_t* values, uint64_t* offsets, uint64_t* win_offsets, uint64_t* win_begin, uint32_t* win_len) {
    if (int rc = translate_args(seq, rec_offsets, n_records, k, codes, values, offsets)) return rc;
    if (!win_offsets) return fail(TXQ_ERR_ARG, "null argument");
    const uint64_t bound = txq_translate_bound(rec_offsets, n_records, k);
    if (bound == UINT64_MAX) return TXQ_ERR_ARG;
    const uint64_t n_win = txq_translate_windows_bound(rec_offsets, n_records, k, window, step);
    if (n_win == UINT64_MAX) return TXQ_ERR_ARG;
    if (n_win > 0xFFFFFFFEull) return fail(TXQ_ERR_ARG, "%llu windows: at most 2^32 - 2 per call", (unsigned long long)n_win);
    const uint64_t first = n_records ? rec_offsets[0] : 0, bytes = n_records ? rec_offsets[n_records] - first : 0;
    if ((bytes && !seq) || (bound && !values) || (n_win && (!win_begin || !win_len))) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = require_init()) return rc;
    const size_t m = 6 * n_records;
    DeviceStage d;  // (+16: the kernels' 16-byte loads of the sequence end inside the slice; +8: no slice of no bytes)
    const size_t s_seq = d.add(bytes + 16), s_rec = d.add((n_records + 1) * 8), s_codes = d.add(256), s_off = d.add((m + 1) * 8), s_val = d.add(bound * 8 + 8);
    const size_t s_woff = d.add((m + 1) * 8), s_wbeg = d.add(n_win * 8 + 8), s_wlen = d.add(n_win * 4 + 8);
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> ro = rebased(rec_offsets, n_records);
    d.upload(s_seq, seq + first, bytes);
    d.upload(s_rec, ro.data(), ro.size() * 8);
    d.upload(s_codes, codes, n_records ? 256 : 0);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_translate_windows_device(d.at<uint8_t>(s_seq), d.at<uint64_t>(s_rec), n_records, k, d.at<uint8_t>(s_codes), window, step, d.at<uint64_t>(s_val),
                                          d.at<uint64_t>(s_off), d.at<uint64_t>(s_woff), d.at<uint64_t>(s_wbeg), d.at<uint32_t>(s_wlen), nullptr);
    if (rc == TXQ_OK) d.download(offsets, s_off, (m + 1) * 8);  // (waits for the kernels)
    if (rc == TXQ_OK && d.error() == hipSuccess) d.download(win_offsets, s_woff, (m + 1) * 8);
    if (rc == TXQ_OK && d.error() == hipSuccess) {
        if (offsets[m] > bound || win_offsets[m] != n_win) rc = fail(TXQ_ERR_OVERFLOW, "translation produced more values or other windows than its bounds");
        else {
            if (offsets[m]) d.download(values, s_val, offsets[m] * 8);
            if (n_win) {
                d.download(win_begin, s_wbeg, n_win * 8);
                d.download(win_len, s_wlen, n_win * 4);
            }
        }
    }
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_translate_windows copies");
    return rc;
}

uint64_t txq_translate_frames_bound(const uint64_t* rec_offsets, size_t n_records) {
    if (n_records && !rec_offsets) {
        (void)fail(TXQ_ERR_ARG, "txq_translate_frames_bound: null offsets");
        return UINT64_MAX;
    }
    if (check_ascending(rec_offsets, n_records, "record")) return UINT64_MAX;
    uint64_t bound = 0;
    for (size_t r = 0; r < n_records; ++r)
        for (uint32_t o = 0; o < 3; ++o) bound += 2 * frame_len(rec_offsets[r + 1] - rec_offsets[r], o);
    return bound;
}

int txq_translate_frames_device(const uint8_t* d_seq, const uint64_t* d_rec_offsets, size_t n_records, uint8_t* d_frames, size_t frames_bytes,
                                uint64_t* d_frame_offsets, void* stream) {
    if (!d_frame_offsets || (n_records && !d_rec_offsets) || (frames_bytes && !d_frames)) return fail(TXQ_ERR_ARG, "null argument");
    (void)d_seq;  // (may be null where there are no bytes: only the caller knows)
    if (n_records > 0x7FFFFFFFull / 6) return fail(TXQ_ERR_ARG, "at most 2^31 / 6 records per call");
    if (int rc = require_init()) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n_records == 0) {
        const hipError_t e = hipMemsetAsync(d_frame_offsets, 0, 8, st);
        return e == hipSuccess ? TXQ_OK : fail_hip(e, "hipMemsetAsync");
    }
    frame_lengths_kernel<<<(unsigned)((n_records + 255) / 256), 256, 0, st>>>(d_rec_offsets, (uint64_t)n_records, d_frame_offsets);
    scan_kernel<<<1, 1024, 0, st>>>(d_frame_offsets + 1, (uint64_t)(6 * n_records));
    frames_kernel<<<kUnits, 64, 0, st>>>(FrArgs{d_seq, d_rec_offsets, (uint64_t)n_records, d_frames, (uint64_t)frames_bytes, d_frame_offsets});
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "translate frames kernel launch");
    return TXQ_OK;
}

int txq_translate_frames(const uint8_t* seq, const uint64_t* rec_offsets, size_t n_records, uint8_t* frames, size_t frames_bytes,
                         uint64_t* frame_offsets) {
    if (!frame_offsets || (n_records && !rec_offsets)) return fail(TXQ_ERR_ARG, "null argument");
    const uint64_t bound = txq_translate_frames_bound(rec_offsets, n_records);
    if (bound == UINT64_MAX) return TXQ_ERR_ARG;
    if (frames_bytes < bound) return fail(TXQ_ERR_ARG, "the frames need %llu bytes, the buffer has %zu", (unsigned long long)bound, frames_bytes);
    const uint64_t first = n_records ? rec_offsets[0] : 0, bytes = n_records ? rec_offsets[n_records] - first : 0;
    if ((bytes && !seq) || (bound && !frames)) return fail(TXQ_ERR_ARG, "null argument");
    if (int rc = require_init()) return rc;
    const size_t m = 6 * n_records;
    DeviceStage d;  // (+16: the kernel's 16-byte loads of the sequence end inside the slice; +8: no slice of no bytes)
    const size_t s_seq = d.add(bytes + 16), s_rec = d.add((n_records + 1) * 8), s_off = d.add((m + 1) * 8), s_frm = d.add(bound + 8);
    if (const hipError_t e = d.alloc(); e != hipSuccess) return fail_hip(e, "hipMalloc");
    const std::vector<uint64_t> ro = n_records ? rebased(rec_offsets, n_records) : std::vector<uint64_t>{0};
    if (bytes) d.upload(s_seq, seq + first, bytes);
    d.upload(s_rec, ro.data(), ro.size() * 8);
    int rc = TXQ_OK;
    if (d.error() == hipSuccess)
        rc = txq_translate_frames_device(d.at<uint8_t>(s_seq), d.at<uint64_t>(s_rec), n_records, d.at<uint8_t>(s_frm), bound, d.at<uint64_t>(s_off), nullptr);
    if (rc == TXQ_OK) d.download(frame_offsets, s_off, (m + 1) * 8);  // (waits for the kernels)
    if (rc == TXQ_OK && d.error() == hipSuccess && bound) d.download(frames, s_frm, bound);
    if (d.error() != hipSuccess) return fail_hip(d.error(), "txq_translate_frames copies");
    return rc;
}

int txq_hit_list_device(const uint64_t* d_hits, const uint32_t* d_counts, size_t n_queries, size_t words, uint32_t* d_list,
                        size_t capacity, uint64_t* d_total, void* stream) {
    if (!d_total || (n_queries && words && !d_hits) || (capacity && !d_list)) return fail(TXQ_ERR_ARG, "null argument");
    if (n_queries >= 0xFFFFFFFFull || words > 0x3FFFFFFull) return fail(TXQ_ERR_ARG, "queries and bins must fit 32 bits");
    if (int rc = require_init()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t m = (uint64_t)n_queries * words;
    if (m == 0) {
        const hipError_t e = hipMemsetAsync(d_total, 0, 8, st);
        return e == hipSuccess ? TXQ_OK : fail_hip(e, "hipMemsetAsync");
    }
    const uint64_t n_tiles = (m + kHitTile - 1) / kHitTile;
    if (n_tiles > 0x7FFFFFFFull) return fail(TXQ_ERR_ARG, "hit matrix too large for one call");
    void* pref = nullptr;
    if (hipError_t e = hipMallocAsync(&pref, (n_tiles + 1) * 8, st); e != hipSuccess) return fail_hip(e, "hipMallocAsync");
    hit_count_kernel<<<(unsigned)n_tiles, kHitThreads, 0, st>>>(d_hits, m, (uint64_t*)pref);
    scan_kernel<<<1, 1024, 0, st>>>((uint64_t*)pref + 1, n_tiles);
    hit_fill_kernel<<<(unsigned)n_tiles, kHitThreads, 0, st>>>(d_hits, d_counts, m, words, (const uint64_t*)pref, n_tiles, d_list, capacity, d_total);
    const hipError_t e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(pref, st);
    if (e != hipSuccess) return fail_hip(e, "hit list kernel launch");
    if (ef != hipSuccess) return fail_hip(ef, "hipFreeAsync");
    return TXQ_OK;
}

}  // extern "C"
