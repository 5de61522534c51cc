// The point sampling rule of the PointRend kernels (pointrend.hip), stated once.
//   point_sample(map, px, py): the map's pixel centres sit at i + 0.5.  fx = px - 0.5, x0 = floor(fx), lx = fx - x0, the same in y; the
//   taps are (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1) with the weights (1-ly)(1-lx), (1-ly)lx, ly(1-lx), ly*lx; a tap outside the map
//   contributes zero and is not read; the four products are summed in that order, in float32 without contraction.
// The 2x upsample of the subdivision uses the same weights and order with the tap indices CLAMPED to the grid (an image resize's
// align_corners=False rule) instead of the zero padding.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

struct PointTaps {
    int x0, y0;                 // the upper-left tap; -2 stands for everything further out (and for a NaN coordinate)
    float w00, w01, w10, w11;   // weights of (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1)
};

// taps of the point (px, py) on a W x H map.  The floor is clamped to [-2, size] in float before the conversion, so no coordinate,
// however large, overflows the integer; every tap of a clamped corner is outside the map.
__host__ __device__ __forceinline__ PointTaps point_taps(float px, float py, int W, int H) {
    const float fx = px - 0.5f, fy = py - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float lx = fx - x0f, ly = fy - y0f;
    PointTaps t;
    t.x0 = (int)fminf(fmaxf(x0f, -2.f), (float)W);
    t.y0 = (int)fminf(fmaxf(y0f, -2.f), (float)H);
    t.w00 = (1.f - ly) * (1.f - lx);
    t.w01 = (1.f - ly) * lx;
    t.w10 = ly * (1.f - lx);
    t.w11 = ly * lx;
    return t;
}

__host__ __device__ __forceinline__ bool point_in(int x, int y, int W, int H) { return x >= 0 && x < W && y >= 0 && y < H; }

// the rule on a scalar map read through at(y, x): products of the taps inside the map, added in tap order
template <typename At>
__host__ __device__ __forceinline__ float point_sample(const PointTaps &t, int W, int H, At at) {
    float s = 0.f;
    if (point_in(t.x0, t.y0, W, H)) s += t.w00 * at(t.y0, t.x0);
    if (point_in(t.x0 + 1, t.y0, W, H)) s += t.w01 * at(t.y0, t.x0 + 1);
    if (point_in(t.x0, t.y0 + 1, W, H)) s += t.w10 * at(t.y0 + 1, t.x0);
    if (point_in(t.x0 + 1, t.y0 + 1, W, H)) s += t.w11 * at(t.y0 + 1, t.x0 + 1);
    return s;
}

// ... and on four adjacent channels of an NHWC map at once (p = the map's (0, 0) pixel at the first of the four channels, ld = floats
// per pixel): the same sum per channel
__device__ __forceinline__ float4 point_sample4(const PointTaps &t, int W, int H, const float *__restrict__ p, size_t ld) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = t.x0 + (k & 1), y = t.y0 + (k >> 1);
        if (!point_in(x, y, W, H)) continue;
        const float w = k == 0 ? t.w00 : k == 1 ? t.w01 : k == 2 ? t.w10 : t.w11;
        const float4 v = ld4(p + ((size_t)y * W + x) * ld);
        s.x += w * v.x; s.y += w * v.y; s.z += w * v.z; s.w += w * v.w;
    }
    return s;
}

// a normalised coordinate from a uint32 key: the upper 24 bits, in [0, 1)
__host__ __device__ __forceinline__ float point_unit(uint32_t key) { return (float)(key >> 8) * 5.9604644775390625e-08f; }

}  // namespace
