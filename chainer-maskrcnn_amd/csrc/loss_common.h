// The two-stage, fixed-order reduction of the loss kernels (loss.hip, box_loss.hip), stated once: every workgroup leaves one (sum, count)
// pair in its partial slot, k_finalize - one wave - adds the slots in double in a fixed order and divides.  No float atomics: the same
// bits on every run.
#pragma once
#include "common.h"
#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int MAXB = 1024;     // partial slots

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// binary cross entropy of logit v against target t in [0, 1] (F.sigmoid_cross_entropy's stable form); gradient sigmoid1(v) - t
__device__ __forceinline__ float bce_logit1(float v, float t) { return -(v * (t - (v >= 0.f ? 1.f : 0.f)) - log1pf(expf(-fabsf(v)))); }

// block-level deterministic sum of (a, b) -> part[blockIdx.x*2 + {0,1}]
__device__ __forceinline__ void block_partial(float a, float b, float *part) {
    __shared__ float sa[NT / 64], sb[NT / 64];
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) { sa[threadIdx.x >> 6] = a; sb[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float x = 0.f, y = 0.f;
        for (int k = 0; k < NT / 64; ++k) { x += sa[k]; y += sb[k]; }
        part[blockIdx.x * 2] = x;
        part[blockIdx.x * 2 + 1] = y;
    }
}

// out[0] = sum(a)/max(sum(b),1), out[1] = max(sum(b),1): one wave, lane l adds partials l, l+64, ... in double,
// then a fixed xor-shuffle tree (bit-reproducible).
__global__ __launch_bounds__(64) void k_finalize(const float *__restrict__ part, int nb, float *__restrict__ out) {
    // (r6) four (sum, count) pairs in flight per lane, four accumulator pairs combined in fixed order: the loop was one dependent load per
    // iteration - up to 64 round trips, 13 us per call on the loss tail of the forward pass; still bit-reproducible)
    const float2 *p2 = reinterpret_cast<const float2 *>(part);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    int k = threadIdx.x;
    for (; k + 192 < nb; k += 256) {
        const float2 v0 = p2[k], v1 = p2[k + 64], v2 = p2[k + 128], v3 = p2[k + 192];
        a0 += (double)v0.x; b0 += (double)v0.y; a1 += (double)v1.x; b1 += (double)v1.y;
        a2 += (double)v2.x; b2 += (double)v2.y; a3 += (double)v3.x; b3 += (double)v3.y;
    }
    for (; k < nb; k += 64) { const float2 v = p2[k]; a0 += (double)v.x; b0 += (double)v.y; }
    double a = (a0 + a1) + (a2 + a3), b = (b0 + b1) + (b2 + b3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if (threadIdx.x == 0) {
        if (b < 1.0) b = 1.0;
        out[0] = (float)(a / b);
        out[1] = (float)b;
    }
}

// one thread per item, at most MAXB workgroups of NT threads: a kernel grid-strides over the rest
int grid_for(long long work) { return (int)std::max(1ll, std::min<long long>((work + NT - 1) / NT, MAXB)); }

}  // namespace
