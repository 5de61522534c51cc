// The arithmetic of GroupNorm in the RoI heads, stated once and shared by the forward and backward kernels of
// groupnorm.hip, register-resident and generic alike, so the ReLU mask the backward recomputes from x is the bits of the forward's
// y > 0 by construction (bn_common.h does the same for BatchNorm; relu1 / relu_mask1 are its rules).  Device only.  No contraction: the
// parenthesisation below IS the rounding order; the one fused operation is the explicit fmaf of the backward sums.
//   statistics  mean = sum(x) / n, var = sum((x - mean)^2) / n about that mean (biased), rstd = 1 / sqrt(var + eps), n = H * W * cpg
//   split statistics (groupnorm_map.hip, DESIGN.md §3.23: the FPN's maps)  a (sample, group) cut into chunks i = 0, 1, ... of n_i elements.
//       Each chunk states its own mean m_i = sum(x) / n_i and M2_i = sum((x - m_i)^2) about it; gn_merge1 folds the chunks in index order
//       (Chan, Golub & LeVeque 1979).  The group's mean is the merged m and its variance M2 / n: a SECOND statement of the mean, equal to
//       sum(x) / n in exact arithmetic and within float32 rounding of it otherwise; still a variance about a mean, never E[x^2] - E[x]^2.
#pragma once
#include "bn_common.h"

#pragma clang fp contract(off)

// 1 / sqrt(var + eps)
__device__ __forceinline__ float gn_rstd1(float var, float eps) { return 1.0f / sqrtf(var + eps); }
// xhat = (v - mean) * rstd
__device__ __forceinline__ float gn_xhat1(float v, float m, float s) { return (v - m) * s; }
// y = gamma * xhat + beta: the layer's value before the ReLU
__device__ __forceinline__ float gn_affine1(float v, float g, float m, float s, float b) { return g * gn_xhat1(v, m, s) + b; }
// acc + gy * xhat in one rounding: one term of sum(gy * xhat)
__device__ __forceinline__ float gn_dot1(float gy, float xh, float acc) { return fmaf(gy, xh, acc); }
// gx = rstd * (gy * gamma - mean_g(gy * gamma) - xhat * mean_g(gy * gamma * xhat))
__device__ __forceinline__ float gn_bwd_dx1(float gy, float xh, float ga, float s, float a, float b) {
    return s * (gy * ga - a - xh * b);
}

// (v - mean)^2: one term of a chunk's M2
__device__ __forceinline__ float gn_sqdev1(float v, float m) {
    const float d = v - m;
    return d * d;
}
// (n, m, M2) of the chunks merged so far takes in chunk i's (ni, mi, M2i); n > 0 and ni > 0
__device__ __forceinline__ void gn_merge1(float &n, float &m, float &M2, float ni, float mi, float M2i) {
    const float nn = n + ni;
    const float d = mi - m;
    m = m + d * ni / nn;
    M2 = M2 + (M2i + d * d * n * ni / nn);
    n = nn;
}

__device__ __forceinline__ float4 gn_sqdev4(const float4 &v, const float4 &m) {
    float4 o; o.x = gn_sqdev1(v.x, m.x); o.y = gn_sqdev1(v.y, m.y); o.z = gn_sqdev1(v.z, m.z); o.w = gn_sqdev1(v.w, m.w);
    return o;
}
__device__ __forceinline__ float4 gn_xhat4(const float4 &v, const float4 &m, const float4 &s) {
    float4 o; o.x = gn_xhat1(v.x, m.x, s.x); o.y = gn_xhat1(v.y, m.y, s.y); o.z = gn_xhat1(v.z, m.z, s.z); o.w = gn_xhat1(v.w, m.w, s.w);
    return o;
}
__device__ __forceinline__ float4 gn_affine4(const float4 &v, const float4 &g, const float4 &m, const float4 &s, const float4 &b) {
    float4 o; o.x = gn_affine1(v.x, g.x, m.x, s.x, b.x); o.y = gn_affine1(v.y, g.y, m.y, s.y, b.y);
    o.z = gn_affine1(v.z, g.z, m.z, s.z, b.z); o.w = gn_affine1(v.w, g.w, m.w, s.w, b.w);
    return o;
}
__device__ __forceinline__ float4 gn_dot4(const float4 &gy, const float4 &xh, const float4 &acc) {
    float4 o; o.x = gn_dot1(gy.x, xh.x, acc.x); o.y = gn_dot1(gy.y, xh.y, acc.y); o.z = gn_dot1(gy.z, xh.z, acc.z);
    o.w = gn_dot1(gy.w, xh.w, acc.w);
    return o;
}
__device__ __forceinline__ float4 gn_bwd_dx4(const float4 &gy, const float4 &xh, const float4 &ga, const float4 &s, const float4 &a,
                                             const float4 &b) {
    float4 o; o.x = gn_bwd_dx1(gy.x, xh.x, ga.x, s.x, a.x, b.x); o.y = gn_bwd_dx1(gy.y, xh.y, ga.y, s.y, a.y, b.y);
    o.z = gn_bwd_dx1(gy.z, xh.z, ga.z, s.z, a.z, b.z); o.w = gn_bwd_dx1(gy.w, xh.w, ga.w, s.w, a.w, b.w);
    return o;
}
// members k of v with keep bit k clear become exact zeros (padded channels)
__device__ __forceinline__ float4 gn_keep4(const float4 &v, unsigned keep) {
    float4 o; o.x = (keep & 1u) ? v.x : 0.f; o.y = (keep & 2u) ? v.y : 0.f; o.z = (keep & 4u) ? v.z : 0.f; o.w = (keep & 8u) ? v.w : 0.f;
    return o;
}
