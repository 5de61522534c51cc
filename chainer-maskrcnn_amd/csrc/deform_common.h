// The deformable-convolution sampling arithmetic, stated once and shared by the three kernels of deform.hip and the
// stand-alone host check tests/native/deform_host_check.cpp.  3x3, stride 1, pad 1, dilation 1, one deformable group.
//   layout     for output pixel (n, y, x) and tap k = 3 * i + j (i, j in 0..2) the offset row holds (dy, dx) in channels 2k, 2k + 1 and,
//              modulated (v2), a logit in channel 18 + k; only these 18 / 27 channels of the padded row are read
//   position   (py, px) = ((y - 1 + i) + dy, (x - 1 + j) + dx), float32
//   sample     the bilinear interpolation of the four cells around it, a cell outside the map counting as zero: a position at or beyond
//              -1 or H (W) samples zero and has a zero gradient; modulated, the sample is multiplied by sigmoid1(logit) (common.h)
//   guard      the position is compared in FLOAT before anything becomes an integer: a huge or non-finite offset (every comparison with a
//              NaN is false) gives valid == 0 and indices 0 - it never indexes memory
//   corners    c = 2 * a + b at (y0 + a, x0 + b), weights w[c] = (a ? ly : hy) * (b ? lx : hx); bit c of ``valid`` = the cell is inside
//   entry      the inverted index of the input gradient names a contribution by e = ((s * 9 + k) * 4 + c), s the flat source pixel:
//              ascending e is ascending (source pixel, tap, corner)
// float32 without contraction.  Restated in torch float64 by tests/deform_reference.py.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DEFORM_HD __host__ __device__
#else
#define DEFORM_HD
#endif

#include <math.h>

#pragma clang fp contract(off)

constexpr int kDeformTaps = 9;           // 3 x 3
constexpr int kDeformOffsetCh = 18;      // (dy, dx) per tap; the v2 logits follow

struct DeformCorners {
    int y0, x0;             // the upper-left cell, in [-1, H - 1] x [-1, W - 1]; 0 when valid == 0
    float ly, lx, hy, hx;   // the fractional parts and 1 - them
    unsigned valid;         // bit 2 * a + b: cell (y0 + a, x0 + b) lies inside the map; 0 = the position samples nothing
};

DEFORM_HD inline DeformCorners deform_corners(float py, float px, int H, int W) {
    DeformCorners t;
    t.y0 = 0; t.x0 = 0; t.ly = 0.f; t.lx = 0.f; t.hy = 0.f; t.hx = 0.f; t.valid = 0u;
    // written so that a NaN fails: inside means -1 < p < H, both strict
    if (!(py > -1.0f && py < (float)H && px > -1.0f && px < (float)W)) return t;
    const float fy = floorf(py), fx = floorf(px);       // in [-1, H - 1]: the conversions below are exact
    t.y0 = (int)fy;
    t.x0 = (int)fx;
    t.ly = py - fy;
    t.lx = px - fx;
    t.hy = 1.0f - t.ly;
    t.hx = 1.0f - t.lx;
    const bool ya = t.y0 >= 0, yb = t.y0 + 1 <= H - 1, xa = t.x0 >= 0, xb = t.x0 + 1 <= W - 1;
    t.valid = (ya && xa ? 1u : 0u) | (ya && xb ? 2u : 0u) | (yb && xa ? 4u : 0u) | (yb && xb ? 8u : 0u);
    return t;
}

DEFORM_HD inline float deform_weight(const DeformCorners &t, int c) { return ((c & 2) ? t.ly : t.hy) * ((c & 1) ? t.lx : t.hx); }

// the sampling position of tap k of output pixel (y, x) under the offsets (dy, dx)
DEFORM_HD inline float deform_pos_y(int y, int k, float dy) { return (float)(y - 1 + k / 3) + dy; }
DEFORM_HD inline float deform_pos_x(int x, int k, float dx) { return (float)(x - 1 + k % 3) + dx; }
