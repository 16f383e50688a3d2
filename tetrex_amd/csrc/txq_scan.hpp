// One-workgroup inclusive scan, shared by the translation units that turn per-item counts into offsets on the device
// (txq_translate.hip: frame and hit-list offsets; txq_edit.hip and txq_regex.hip: the pairs' work units).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace txq {
namespace {

// Inclusive scan of x[0 .. m) in place by one workgroup: 8 entries per thread and round.
__global__ __launch_bounds__(1024) void scan_kernel(uint64_t* x, uint64_t m) {
    __shared__ uint64_t wsum[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < m; t0 += 8192) {
        const uint64_t i0 = t0 + (uint64_t)threadIdx.x * 8;
        uint64_t v[8], sum = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = i0 + e < m ? x[i0 + e] : 0;
            sum += v[e];
        }
        uint64_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up(incl, d);
            if ((int)lane >= d) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        uint64_t run = carry + before + incl - sum;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            run += v[e];
            if (i0 + e < m) x[i0 + e] = run;
        }
        carry += total;
        __syncthreads();
    }
}

}  // namespace
}  // namespace txq
