// The arithmetic of BatchNorm in the training step, stated once and shared by the training-mode and inference-mode
// kernels of nn.hip, the frozen-layer kernels of bn_frozen.hip and the BatchNorm + ReLU on load of conv.hip's Winograd input transform,
// so a value any of them recomputes (a ReLU mask from x, a normalised tap, the two layers of a pair) is the bits the forward kernel wrote,
// by construction.  Device only.  Each rule is one scalar function; its 4-wide form applies it to the members x, y, z, w of a float4, one
// member after the other (conv.hip, whose taps are not float4, calls the scalar rules).  The 4-wide forms take references: by-value
// float4 parameters change how the callers are vectorised.  No contraction: the parenthesisation below IS the rounding order; the one
// fused operation is the explicit fmaf of the backward sums.
//   forward    chainer.functions.batch_normalization / fixed_batch_normalization (eps 2e-5) as ResNet50Layers uses them,
//              chainer_maskrcnn/model/extractor/feature_pyramid_network.py:48-66
#pragma once
#include "common.h"

#pragma clang fp contract(off)

// 1 / sqrt(var + eps): the inverse standard deviation from a (running) variance
__device__ __forceinline__ float bn_inv_std1(float var, float eps) { return 1.0f / sqrtf(var + eps); }
// xhat = (v - mean) * invstd
__device__ __forceinline__ float bn_xhat1(float v, float m, float s) { return (v - m) * s; }
// y = gamma * xhat + beta: the layer's value before residual / ReLU
__device__ __forceinline__ float bn_affine1(float v, float g, float m, float s, float b) { return g * bn_xhat1(v, m, s) + b; }
// ReLU: max(o, 0)
__device__ __forceinline__ float relu1(float o) { return fmaxf(o, 0.f); }
// ReLU backward: g where the forward's output y is > 0, else 0
__device__ __forceinline__ float relu_mask1(float g, float y) { return y > 0.f ? g : 0.f; }
// acc + g * xhat in one rounding: one term of sum(dz * xhat)
__device__ __forceinline__ float bn_dot1(float g, float v, float m, float s, float acc) { return fmaf(g, bn_xhat1(v, m, s), acc); }
// gx = gamma * invstd * (dz - gbeta / P - xhat * (ggamma / P)), invP = 1 / P
__device__ __forceinline__ float bn_bwd_dx1(float g, float v, float ga, float m, float s, float gb, float gg, float invP) {
    return ga * s * (g - gb * invP - bn_xhat1(v, m, s) * (gg * invP));
}

__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) {
    float4 o; o.x = a.x + b.x; o.y = a.y + b.y; o.z = a.z + b.z; o.w = a.w + b.w;
    return o;
}
__device__ __forceinline__ float4 mul4(const float4 &a, const float4 &b) {
    float4 o; o.x = a.x * b.x; o.y = a.y * b.y; o.z = a.z * b.z; o.w = a.w * b.w;
    return o;
}
__device__ __forceinline__ float4 relu4(const float4 &v) {
    float4 o = v;
    o.x = relu1(o.x); o.y = relu1(o.y); o.z = relu1(o.z); o.w = relu1(o.w);
    return o;
}
__device__ __forceinline__ float4 relu_mask4(const float4 &g, const float4 &y) {
    float4 o = g;
    o.x = relu_mask1(o.x, y.x); o.y = relu_mask1(o.y, y.y); o.z = relu_mask1(o.z, y.z); o.w = relu_mask1(o.w, y.w);
    return o;
}
__device__ __forceinline__ float4 bn_inv_std4(const float4 &var, float eps) {
    float4 o; o.x = bn_inv_std1(var.x, eps); o.y = bn_inv_std1(var.y, eps); o.z = bn_inv_std1(var.z, eps); o.w = bn_inv_std1(var.w, eps);
    return o;
}
__device__ __forceinline__ float4 bn_affine4(const float4 &v, const float4 &g, const float4 &m, const float4 &s, const float4 &b) {
    float4 o; o.x = bn_affine1(v.x, g.x, m.x, s.x, b.x); o.y = bn_affine1(v.y, g.y, m.y, s.y, b.y);
    o.z = bn_affine1(v.z, g.z, m.z, s.z, b.z); o.w = bn_affine1(v.w, g.w, m.w, s.w, b.w);
    return o;
}
__device__ __forceinline__ float4 bn_dot4(const float4 &g, const float4 &v, const float4 &m, const float4 &s, const float4 &acc) {
    float4 o = acc;
    o.x = bn_dot1(g.x, v.x, m.x, s.x, o.x); o.y = bn_dot1(g.y, v.y, m.y, s.y, o.y);
    o.z = bn_dot1(g.z, v.z, m.z, s.z, o.z); o.w = bn_dot1(g.w, v.w, m.w, s.w, o.w);
    return o;
}
// one element of the backward partial sums: a = sum(dz) += g, b = sum(dz * xhat) = fma(g, xhat, b)
__device__ __forceinline__ void bn_bwd_acc4(const float4 &g, const float4 &v, const float4 &m, const float4 &s, float4 &a, float4 &b) {
    a = add4(a, g);
    b = bn_dot4(g, v, m, s, b);
}
__device__ __forceinline__ float4 bn_bwd_dx4(const float4 &g, const float4 &v, const float4 &ga, const float4 &m, const float4 &s,
                                             const float4 &gb, const float4 &gg, float invP) {
    float4 o; o.x = bn_bwd_dx1(g.x, v.x, ga.x, m.x, s.x, gb.x, gg.x, invP); o.y = bn_bwd_dx1(g.y, v.y, ga.y, m.y, s.y, gb.y, gg.y, invP);
    o.z = bn_bwd_dx1(g.z, v.z, ga.z, m.z, s.z, gb.z, gg.z, invP); o.w = bn_bwd_dx1(g.w, v.w, ga.w, m.w, s.w, gb.w, gg.w, invP);
    return o;
}
// a = gamma * (1 / sqrt(var + eps)): the per-channel scale a frozen layer's backward multiplies by
__device__ __forceinline__ float4 bn_scale4(const float4 &g, const float4 &var, float eps) { return mul4(g, bn_inv_std4(var, eps)); }
