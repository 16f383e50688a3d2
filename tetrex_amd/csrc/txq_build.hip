// Index construction kernels for gfx950 (`tetrex index --layout sized`, host/layout.hpp): HyperLogLog sketches of the
// user bins, the table of union estimates the layout DP reads, and the insertion of every k-mer into each IBF on its user
// bin's path.  The hash, the registers and the estimator are defined exactly (include/txq.h) so that a numpy restatement
// matches them bit for bit (tests/test_gpu_sized_hibf.py; each kernel alone at its edges: tests/test_gpu_build_kernels.py).
#include "txq_internal.hpp"

#include <cmath>
#include <mutex>

namespace txq {

namespace {

constexpr uint32_t kHllBits = TXQ_HLL_BITS;
constexpr uint32_t kRegs = TXQ_HLL_REGISTERS;
constexpr uint32_t kSketchThreads = 256;
constexpr uint32_t kSketchSlices = 16;        // workgroups per bin at most ...
constexpr uint64_t kSketchMinSlice = 16384;   // ... each with at least this many values (small bins: one workgroup)
constexpr uint32_t kUnionThreads = 256;       // 16 registers per lane
constexpr uint32_t kRegsPerLane = kRegs / kUnionThreads;
constexpr uint32_t kPairThreads = 256;        // pair unions: four waves, each with whole bins (64 registers per lane)
constexpr uint32_t kPairTile = 16;            // a workgroup's tile: 16 x 16 pairs
constexpr uint32_t kPairRows = kPairTile / (kPairThreads / 64);  // row bins a wave keeps in VGPRs (4 x 16 u32)
constexpr uint32_t kPairQuads = kRegs / 16 / 64;                 // uint4 per lane and bin (4)
constexpr uint64_t kPairMaxBins = 4096;

// linear counting m * ln(m / V), V = 0 .. m, filled on the host (one libm for the device and for restatements)
__constant__ double kLinearCount[kRegs + 1];

__device__ __forceinline__ uint64_t fmix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// one workgroup per (bin, slice): registers in LDS (ds_max_u32), merged into u32 registers in HBM
__global__ __launch_bounds__(kSketchThreads) void sketch_kernel(const uint64_t* __restrict__ values, size_t n_values,
                                                                const uint64_t* __restrict__ offsets, uint32_t* __restrict__ regs32) {
    __shared__ uint32_t reg[kRegs];
    const uint64_t bin = blockIdx.x / kSketchSlices, slice = blockIdx.x % kSketchSlices;
    const uint64_t lo = offsets[bin], hi = min((uint64_t)n_values, offsets[bin + 1]);
    if (hi <= lo) return;
    const uint64_t len = hi - lo;
    const uint64_t chunk = max(kSketchMinSlice, (len + kSketchSlices - 1) / kSketchSlices);
    const uint64_t a = lo + slice * chunk;
    if (slice * chunk >= len) return;  // uniform over the workgroup
    const uint64_t b = min(hi, a + chunk);
    for (uint32_t r = threadIdx.x; r < kRegs; r += kSketchThreads) reg[r] = 0;
    __syncthreads();
    for (uint64_t i = a + threadIdx.x; i < b; i += kSketchThreads) {
        const uint64_t x = fmix64(values[i]);
        const uint32_t rank = min((uint32_t)__clzll(x << kHllBits), 64u - kHllBits) + 1;
        atomicMax(&reg[x >> (64 - kHllBits)], rank);
    }
    __syncthreads();
    uint32_t* out = regs32 + bin * kRegs;
    for (uint32_t r = threadIdx.x; r < kRegs; r += kSketchThreads)
        if (reg[r]) atomicMax(&out[r], reg[r]);
}

__global__ __launch_bounds__(256) void narrow_kernel(const uint32_t* __restrict__ regs32, uint8_t* __restrict__ regs8, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        regs8[i] = (uint8_t)max((uint32_t)regs8[i], regs32[i]);  // max with what earlier chunks left
}

// one workgroup per start position s: the running max of bins order[s .. s+L-1] in VGPRs (16 registers per lane),
// sum_r 2^-M[r] as the exact integer sum_r 2^(53 - M[r]) (split in 32-bit halves so no partial sum overflows)
__global__ __launch_bounds__(kUnionThreads) void union_kernel(const uint8_t* __restrict__ regs, const uint32_t* __restrict__ order,
                                                              uint64_t n_bins, uint32_t window, double alpha_mm,
                                                              double* __restrict__ est) {
    __shared__ uint64_t part[3][kUnionThreads / 64];
    const uint64_t s = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t m[kRegsPerLane / 4] = {0, 0, 0, 0};  // 16 u8 registers, four per u32
    for (uint32_t L = 1; L <= window; ++L) {
        if (s + L > n_bins) {  // uniform: past the end of the order
            if (threadIdx.x == 0) est[s * window + L - 1] = 0.0;
            continue;
        }
        const uint32_t b = order[s + L - 1];
        const uint4 v = *reinterpret_cast<const uint4*>(regs + (uint64_t)b * kRegs + threadIdx.x * kRegsPerLane);
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
        uint64_t sum = 0, zeros = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            uint32_t acc = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t r = max((m[w] >> (8 * k)) & 0xFFu, (in[w] >> (8 * k)) & 0xFFu);
                acc |= r << (8 * k);
                sum += 1ULL << (53 - min(r, 53u));
                zeros += r == 0;
            }
            m[w] = acc;
        }
        uint64_t lo = sum & 0xFFFFFFFFull, hi = sum >> 32;
        for (int o = 32; o > 0; o >>= 1) {
            lo += __shfl_xor(lo, o);
            hi += __shfl_xor(hi, o);
            zeros += __shfl_xor(zeros, o);
        }
        if (lane == 0) { part[0][wave] = lo; part[1][wave] = hi; part[2][wave] = zeros; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t tl = 0, th = 0, tz = 0;
            for (uint32_t w = 0; w < kUnionThreads / 64; ++w) { tl += part[0][w]; th += part[1][w]; tz += part[2][w]; }
            const double z = ((double)th * 4294967296.0 + (double)tl) * 0x1p-53;
            double e = alpha_mm / z;
            if (e <= 2.5 * kRegs && tz > 0) e = kLinearCount[tz];
            est[s * window + L - 1] = e;
        }
        __syncthreads();
    }
}

// Pair unions: one workgroup per 16 x 16 tile of pairs (i, j) with tile column >= tile row; both halves of the matrix are
// written.  A lane only ever needs its own 64 registers of a bin (uint4 q * 64 + lane, q = 0 .. 3, coalesced), so the tile's
// 16 row bins live in VGPRs, four per wave, and its 16 column bins are staged once in LDS (64 KiB: two workgroups per
// CU) where all four waves read them: 256 B of global reads per pair.  Per pair a wave takes the byte-wise max of its
// lanes' registers, sums 2^(53 - M) exactly as union_kernel does, and reduces with shuffles; no cross-wave step.
__global__ __launch_bounds__(kPairThreads) void pair_union_kernel(const uint8_t* __restrict__ regs, const uint32_t* __restrict__ ids,
                                                                   uint32_t n, double alpha_mm, double* __restrict__ est) {
    __shared__ uint4 cols[kPairTile][kRegs / 16];
    const uint32_t ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;  // uniform: the lower triangle is written by its mirror tile
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // bins past n are never computed (the loops below stop at n): their slots load bin n - 1, a valid address
#pragma unroll 4
    for (uint32_t jj = 0; jj < kPairTile; ++jj) {
        const uint32_t gj = min(tj * kPairTile + jj, n - 1);
        cols[jj][threadIdx.x] = reinterpret_cast<const uint4*>(regs + (uint64_t)ids[gj] * kRegs)[threadIdx.x];
    }
    uint32_t a[kPairRows][kPairQuads * 4];
#pragma unroll
    for (uint32_t ii = 0; ii < kPairRows; ++ii) {
        const uint32_t gi = min(ti * kPairTile + wave * kPairRows + ii, n - 1);
#pragma unroll
        for (uint32_t q = 0; q < kPairQuads; ++q) {
            const uint4 v = reinterpret_cast<const uint4*>(regs + (uint64_t)ids[gi] * kRegs)[q * 64 + lane];
            a[ii][4 * q] = v.x; a[ii][4 * q + 1] = v.y; a[ii][4 * q + 2] = v.z; a[ii][4 * q + 3] = v.w;
        }
    }
    __syncthreads();
    for (uint32_t jj = 0; jj < kPairTile; ++jj) {
        const uint32_t gj = tj * kPairTile + jj;
        if (gj >= n) break;  // uniform
        uint32_t b[kPairQuads * 4];
#pragma unroll
        for (uint32_t q = 0; q < kPairQuads; ++q) {
            const uint4 v = cols[jj][q * 64 + lane];
            b[4 * q] = v.x; b[4 * q + 1] = v.y; b[4 * q + 2] = v.z; b[4 * q + 3] = v.w;
        }
#pragma unroll
        for (uint32_t ii = 0; ii < kPairRows; ++ii) {
            const uint32_t gi = ti * kPairTile + wave * kPairRows + ii;
            if (gi >= n) continue;  // uniform over the wave
            uint64_t sum = 0;
            uint32_t zeros = 0;
#pragma unroll
            for (uint32_t w = 0; w < kPairQuads * 4; ++w) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t r = max((a[ii][w] >> (8 * k)) & 0xFFu, (b[w] >> (8 * k)) & 0xFFu);
                    sum += 1ULL << (53 - min(r, 53u));
                    zeros += r == 0;
                }
            }
            uint32_t lo = (uint32_t)sum, hi = (uint32_t)(sum >> 32);  // a lane's 64 registers: sum < 2^60
            uint64_t tl = lo, th = hi;
            for (int o = 32; o > 0; o >>= 1) {
                tl += __shfl_xor(tl, o);
                th += __shfl_xor(th, o);
                zeros += __shfl_xor(zeros, o);
            }
            if (lane == 0) {
                const double z = ((double)th * 4294967296.0 + (double)tl) * 0x1p-53;
                double e = alpha_mm / z;
                if (e <= 2.5 * kRegs && zeros > 0) e = kLinearCount[zeros];
                est[(uint64_t)gi * n + gj] = e;
                if (ti != tj) est[(uint64_t)gj * n + gi] = e;
            }
        }
    }
}

struct PathEntry {
    uint64_t ibf, tb, parts;
};

// one lane per value: every IBF on its user bin's path gets the value in the technical bin (of a split bin: the part) that
// holds it — h bits per IBF, set with atomicOr (idempotent, order-free)
__global__ __launch_bounds__(256) void tree_insert_kernel(const uint64_t* __restrict__ values, size_t n_values,
                                                          const uint64_t* __restrict__ offsets, uint64_t n_bins,
                                                          const uint64_t* __restrict__ path_offsets, const PathEntry* __restrict__ path,
                                                          const txq_ibf_desc* __restrict__ ibfs, uint64_t n_ibf) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_values; i += stride) {
        uint64_t l = 0, r = n_bins;  // the bin b with offsets[b] <= i < offsets[b + 1]
        while (r - l > 1) {
            const uint64_t mid = (l + r) >> 1;
            if (offsets[mid] <= i) l = mid; else r = mid;
        }
        if (i < offsets[l] || i >= offsets[l + 1]) continue;
        const uint64_t v = values[i];
        const uint64_t part_hash = fmix64(v ^ 0x9e3779b97f4a7c15ULL);
        for (uint64_t e = path_offsets[l]; e < path_offsets[l + 1]; ++e) {
            const PathEntry p = path[e];
            if (p.ibf >= n_ibf) continue;
            const txq_ibf_desc f = ibfs[p.ibf];
            const uint64_t tb = p.tb + (p.parts > 1 ? __umul64hi(part_hash, p.parts) : 0);
            if (tb >= f.bins || f.bin_size == 0 || tb / 64 >= f.bin_words) continue;
            const uint32_t shift = (uint32_t)f.hash_shift, h = (uint32_t)min(f.hash_funs, (uint64_t)5);
            unsigned long long* words = (unsigned long long*)f.words;
            for (uint32_t j = 0; j < h; ++j) {
                const uint64_t row = hash_row(v, kSeeds[j], shift, f.bin_size);
                atomicOr(words + row * f.bin_words + tb / 64, 1ULL << (tb & 63));
            }
        }
    }
}

unsigned grid_for(size_t n, unsigned per_block) {
    const size_t blocks = (n + per_block - 1) / per_block;
    return (unsigned)std::min<size_t>(std::max<size_t>(blocks, 1), 256 * 256);
}

int upload_linear_count(hipStream_t st) {
    static double table[kRegs + 1];
    static std::once_flag once;
    std::call_once(once, [] {
        table[0] = 0.0;
        for (uint32_t v = 1; v <= kRegs; ++v) table[v] = (double)kRegs * std::log((double)kRegs / (double)v);
    });
    const hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(kLinearCount), table, sizeof table, 0, hipMemcpyHostToDevice, st);
    return e == hipSuccess ? TXQ_OK : fail_hip(e, "linear counting table");
}

}  // namespace

}  // namespace txq

using namespace txq;

extern "C" {

int txq_sketch_device(const uint64_t* d_values, size_t n_values, const uint64_t* d_offsets, uint64_t n_bins, uint8_t* d_registers,
                      void* stream) {
    if (int rc = require_init()) return rc;
    if (n_bins == 0) return TXQ_OK;
    if (!d_offsets || !d_registers || (n_values && !d_values)) return fail(TXQ_ERR_ARG, "null argument");
    if (n_bins * kSketchSlices > 0x7FFFFFFFull) return fail(TXQ_ERR_ARG, "too many bins for one sketch launch");
    hipStream_t st = (hipStream_t)stream;
    const size_t n_regs = (size_t)n_bins * kRegs;
    void* regs32 = nullptr;
    if (hipError_t e = hipMallocAsync(&regs32, n_regs * 4, st); e != hipSuccess) return fail_hip(e, "hipMallocAsync");
    hipError_t e = hipMemsetAsync(regs32, 0, n_regs * 4, st);
    if (e == hipSuccess) {
        sketch_kernel<<<(unsigned)(n_bins * kSketchSlices), kSketchThreads, 0, st>>>(d_values, n_values, d_offsets, (uint32_t*)regs32);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        narrow_kernel<<<grid_for(n_regs, 256), 256, 0, st>>>((const uint32_t*)regs32, d_registers, n_regs);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(regs32, st);
    if (e != hipSuccess) return fail_hip(e, "sketch kernels");
    if (ef != hipSuccess) return fail_hip(ef, "hipFreeAsync");
    return TXQ_OK;
}

int txq_union_estimates_device(const uint8_t* d_registers, const uint32_t* d_order, uint64_t n_bins, uint64_t window,
                               double* d_estimates, void* stream) {
    if (int rc = require_init()) return rc;
    if (n_bins == 0) return TXQ_OK;
    if (!d_registers || !d_order || !d_estimates) return fail(TXQ_ERR_ARG, "null argument");
    if (window < 1 || window > n_bins || n_bins > 0x7FFFFFFFull) return fail(TXQ_ERR_ARG, "window must lie in 1 .. n_bins");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_linear_count(st)) return rc;
    const double m = kRegs, alpha_mm = 0.7213 / (1.0 + 1.079 / m) * m * m;
    union_kernel<<<(unsigned)n_bins, kUnionThreads, 0, st>>>(d_registers, d_order, n_bins, (uint32_t)window, alpha_mm, d_estimates);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "union estimate kernel launch");
    return TXQ_OK;
}

int txq_pair_unions_device(const uint8_t* d_registers, const uint32_t* d_ids, uint64_t n, double* d_estimates, void* stream) {
    if (int rc = require_init()) return rc;
    if (n == 0) return TXQ_OK;
    if (!d_registers || !d_ids || !d_estimates) return fail(TXQ_ERR_ARG, "null argument");
    if (n > kPairMaxBins) return fail(TXQ_ERR_ARG, "at most 4096 bins per pair table");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_linear_count(st)) return rc;
    const double m = kRegs, alpha_mm = 0.7213 / (1.0 + 1.079 / m) * m * m;
    const unsigned tiles = (unsigned)((n + kPairTile - 1) / kPairTile);
    pair_union_kernel<<<dim3(tiles, tiles), kPairThreads, 0, st>>>(d_registers, d_ids, (uint32_t)n, alpha_mm, d_estimates);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "pair union kernel launch");
    return TXQ_OK;
}

int txq_tree_insert_device(const uint64_t* d_values, size_t n_values, const uint64_t* d_offsets, uint64_t n_bins,
                           const uint64_t* d_path_offsets, const uint64_t* d_path, const txq_ibf_desc* d_ibfs, uint64_t n_ibf,
                           void* stream) {
    if (int rc = require_init()) return rc;
    if (n_values == 0 || n_bins == 0) return TXQ_OK;
    if (!d_values || !d_offsets || !d_path_offsets || !d_path || !d_ibfs) return fail(TXQ_ERR_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    tree_insert_kernel<<<grid_for(n_values, 256), 256, 0, st>>>(d_values, n_values, d_offsets, n_bins, d_path_offsets,
                                                                (const PathEntry*)d_path, d_ibfs, n_ibf);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "tree insert kernel launch");
    return TXQ_OK;
}

}  // extern "C"
