// Frozen BatchNorm in the training step, and the MomentumSGD update that leaves frozen parameters alone (gfx950, NHWC fp32).
//
// A frozen BatchNorm is the inference-mode layer of nn.hip (k_bn_infer: running statistics, constant affine) used inside the training
// step: its forward pass IS mrcnn_bn_infer_fwd_f32; this file adds what the step needs around it -
//   k_bn_frozen_bwd        gx = dz * a[c], a[c] = gamma[c] * (1.0f / sqrtf(avg_var[c] + eps)), dz = gy under the layer's ReLU mask;
//   k_bn_infer_pair        relu(bn_a(xa) + bn_b(xb)): main branch + projection shortcut of a bottleneck in one apply;
//   k_bn_frozen_bwd_pair   both input gradients of that pair from one read of gy (and y);
//   k_sgd_masked           k_sgd over a section of the flat parameter buffer, skipping the 64-float blocks of frozen parameters.
// No statistics, no reductions, no workspace, no atomics: every kernel streams float4, each tensor byte crosses HBM once.
// Algorithmic bytes per element: bwd 12 with a mask stream (y or x), 8 without; pair fwd 12; pair bwd 16 (12 when gy arrives masked);
// sgd 20 per trainable parameter, 0 per frozen one.
//
// The per-channel coefficient costs a correctly rounded square root and division.  A thread's channel group is the same in every
// iteration of its grid-stride loop whenever C/4 divides the stride (every power-of-two C up to 4 * stride - all ResNet widths): the
// coefficients are then computed once per thread, otherwise once per element.  Same expression either way, hence the same bits.
// (The stride is at most 4096 * 256 and a thread's first element lies below it: those two remainders are 32-bit; the 64-bit remainder of
// the per-element path is ~150 instructions of software division, as everywhere in nn.hip's grid-stride kernels.)
#include "common.h"
#include "bn_common.h"
#include <algorithm>

namespace {

constexpr int NT = 256;

inline int ew_grid(size_t n4) { return (int)std::min<size_t>((n4 + NT - 1) / NT, 256 * 16); }

// MODE 0: dz = gy.  1: dz = gy where y > 0 (yx = y).  2: dz = gy where the forward's y, recomputed from yx = x, is > 0.
// gx may be gy (every element is read before it is written, by the same thread).
template <int MODE>
__global__ __launch_bounds__(NT) void k_bn_frozen_bwd(const float *gy, const float *__restrict__ yx, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, const float *__restrict__ mean,
                                                      const float *__restrict__ var, float *gx, float *__restrict__ gres, size_t n4,
                                                      int C4, float eps) {
    const size_t stride = (size_t)gridDim.x * NT;
    size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    const bool fixed = ((unsigned)stride % (unsigned)C4) == 0;         // grid-uniform
    float4 a, s, g_, m, b;
    auto coef = [&](int c) {
        g_ = ld4(gamma + c);
        a = bn_scale4(g_, ld4(var + c), eps);
        if (MODE == 2) { s = bn_inv_std4(ld4(var + c), eps); m = ld4(mean + c); b = ld4(beta + c); }
    };
    if (fixed) coef((int)((unsigned)i % (unsigned)C4) * 4);
    for (; i < n4; i += stride) {
        if (!fixed) coef((int)(i % C4) * 4);
        float4 g = ld4s(gy + i * 4);
        if (MODE == 1) g = relu_mask4(g, ld4s(yx + i * 4));
        if (MODE == 2) g = relu_mask4(g, bn_affine4(ld4s(yx + i * 4), g_, m, s, b));
        st4(gx + i * 4, mul4(g, a));
        if (gres) st4(gres + i * 4, g);
    }
}

// y = relu(bn_a(xa) + bn_b(xb)), evaluated as r = bn_b(xb) first, then bn_a(xa) + r: the bits of the two single-layer calls.
__global__ __launch_bounds__(NT) void k_bn_infer_pair(const float *__restrict__ xa, const float *__restrict__ gamma_a,
                                                      const float *__restrict__ beta_a, const float *__restrict__ mean_a,
                                                      const float *__restrict__ var_a, const float *__restrict__ xb,
                                                      const float *__restrict__ gamma_b, const float *__restrict__ beta_b,
                                                      const float *__restrict__ mean_b, const float *__restrict__ var_b,
                                                      float *__restrict__ y, size_t n4, int C4, float eps) {
    const size_t stride = (size_t)gridDim.x * NT;
    size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    const bool fixed = ((unsigned)stride % (unsigned)C4) == 0;
    float4 ga, ba, ma, sa, gb, bb, mb, sb;
    auto coef = [&](int c) {
        ga = ld4(gamma_a + c); ba = ld4(beta_a + c); ma = ld4(mean_a + c); sa = bn_inv_std4(ld4(var_a + c), eps);
        gb = ld4(gamma_b + c); bb = ld4(beta_b + c); mb = ld4(mean_b + c); sb = bn_inv_std4(ld4(var_b + c), eps);
    };
    if (fixed) coef((int)((unsigned)i % (unsigned)C4) * 4);
    for (; i < n4; i += stride) {
        if (!fixed) coef((int)(i % C4) * 4);
        const float4 va = ld4s(xa + i * 4), vb = ld4s(xb + i * 4);
        const float4 r = bn_affine4(vb, gb, mb, sb, bb);
        st4(y + i * 4, relu4(add4(bn_affine4(va, ga, ma, sa, ba), r)));
    }
}

// dz = y ? gy where y > 0 : gy; gxa = dz * a_a, gxb = dz * a_b.  gxa or gxb may be gy.
__global__ __launch_bounds__(NT) void k_bn_frozen_bwd_pair(const float *gy, const float *__restrict__ y, const float *__restrict__ gamma_a,
                                                           const float *__restrict__ var_a, const float *__restrict__ gamma_b,
                                                           const float *__restrict__ var_b, float *gxa, float *gxb, size_t n4, int C4,
                                                           float eps) {
    const size_t stride = (size_t)gridDim.x * NT;
    size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n4) return;
    const bool fixed = ((unsigned)stride % (unsigned)C4) == 0;
    float4 aa, ab;
    auto coef = [&](int c) { aa = bn_scale4(ld4(gamma_a + c), ld4(var_a + c), eps); ab = bn_scale4(ld4(gamma_b + c), ld4(var_b + c), eps); };
    if (fixed) coef((int)((unsigned)i % (unsigned)C4) * 4);
    for (; i < n4; i += stride) {
        if (!fixed) coef((int)(i % C4) * 4);
        float4 g = ld4s(gy + i * 4);
        if (y) g = relu_mask4(g, ld4s(y + i * 4));
        st4(gxa + i * 4, mul4(g, aa));
        st4(gxb + i * 4, mul4(g, ab));
    }
}

// k_sgd (nn.hip) on the elements [0, n) of a section whose first element is element `offset` of the flat buffer:
// v = momentum*v - lr*(g + wd*p); p += v, except in 64-float blocks whose bit is set in `frozen` (bit b of word b / 32 = block b of
// the flat buffer): those are neither read nor written.  float4 groups are aligned to the FLAT buffer (a group never straddles a block);
// the up to 3 elements in front of the first group and behind the last one go one by one.
__device__ __forceinline__ bool is_frozen(const uint32_t *__restrict__ frozen, size_t elem) {
    const size_t blk = elem >> 6;
    return (frozen[blk >> 5] >> (blk & 31)) & 1u;
}
__global__ __launch_bounds__(NT) void k_sgd_masked(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ v, size_t n,
                                                   size_t offset, const uint32_t *__restrict__ frozen, float lr, float momentum, float wd) {
    const size_t lead = (4 - (offset & 3)) & 3, head = lead < n ? lead : n;
    const size_t n4 = (n - head) / 4;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
        const size_t e = head + i * 4;
        if (is_frozen(frozen, offset + e)) continue;
        float4 pp = ld4(p + e), vv = ld4(v + e);
        const float4 gg = ld4(g + e);
        vv.x = momentum * vv.x - lr * (gg.x + wd * pp.x); vv.y = momentum * vv.y - lr * (gg.y + wd * pp.y);
        vv.z = momentum * vv.z - lr * (gg.z + wd * pp.z); vv.w = momentum * vv.w - lr * (gg.w + wd * pp.w);
        pp.x += vv.x; pp.y += vv.y; pp.z += vv.z; pp.w += vv.w;
        st4(p + e, pp);
        st4(v + e, vv);
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const size_t tail0 = head + n4 * 4;
        const size_t e = threadIdx.x < 4 ? (size_t)threadIdx.x : tail0 + (threadIdx.x - 4);
        const bool mine = threadIdx.x < 4 ? (size_t)threadIdx.x < head : e < n;
        if (mine && !is_frozen(frozen, offset + e)) {
            const float nv = momentum * v[e] - lr * (g[e] + wd * p[e]);
            v[e] = nv;
            p[e] += nv;
        }
    }
}

int chk(bool ok, const char *what) { return ok ? 0 : mrcnn::fail_arg(MRCNN_E_INVALID, "%s", what); }
bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mrcnn_bn_frozen_bwd_f32(const float *gy, const float *yx, const float *gamma, const float *beta, const float *avg_mean,
                                       const float *avg_var, float *gx, float *gres, int P, int C, float eps, int relu, void *stream) {
    if (int e = chk(gy && gamma && avg_var && gx, "bn_frozen_bwd: null pointer")) return e;
    if (int e = chk(relu >= 0 && relu <= 2, "bn_frozen_bwd: relu is 0 (no mask), 1 (mask from y) or 2 (mask recomputed from x)")) return e;
    if (int e = chk(relu == 0 || yx, "bn_frozen_bwd: relu 1 / 2 need the y / x tensor")) return e;
    if (int e = chk(relu != 2 || (beta && avg_mean), "bn_frozen_bwd: relu 2 needs beta and avg_mean")) return e;
    if (int e = chk(P > 0 && C > 0 && (C % 4) == 0, "bn_frozen_bwd: need P>0, C%4==0")) return e;
    if (int e = chk(al16(gy) && al16(yx) && al16(gamma) && al16(beta) && al16(avg_mean) && al16(avg_var) && al16(gx) && al16(gres),
                    "bn_frozen_bwd: pointers must be 16-byte aligned")) return e;
    if (int e = chk(gres == nullptr || (gres != gy && gres != gx), "bn_frozen_bwd: gres must be a buffer of its own")) return e;
    const size_t n4 = (size_t)P * C / 4;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ew_grid(n4)), block(NT);
    if (relu == 0) hipLaunchKernelGGL(k_bn_frozen_bwd<0>, grid, block, 0, st, gy, yx, gamma, beta, avg_mean, avg_var, gx, gres, n4, C / 4, eps);
    else if (relu == 1) hipLaunchKernelGGL(k_bn_frozen_bwd<1>, grid, block, 0, st, gy, yx, gamma, beta, avg_mean, avg_var, gx, gres, n4, C / 4, eps);
    else hipLaunchKernelGGL(k_bn_frozen_bwd<2>, grid, block, 0, st, gy, yx, gamma, beta, avg_mean, avg_var, gx, gres, n4, C / 4, eps);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_bn_infer_fwd_pair_f32(const float *xa, const float *gamma_a, const float *beta_a, const float *mean_a,
                                           const float *var_a, const float *xb, const float *gamma_b, const float *beta_b,
                                           const float *mean_b, const float *var_b, float *y, int P, int C, float eps, void *stream) {
    if (int e = chk(xa && gamma_a && beta_a && mean_a && var_a && xb && gamma_b && beta_b && mean_b && var_b && y,
                    "bn_infer_fwd_pair: null pointer")) return e;
    if (int e = chk(P > 0 && C > 0 && (C % 4) == 0, "bn_infer_fwd_pair: need P>0, C%4==0")) return e;
    if (int e = chk(al16(xa) && al16(gamma_a) && al16(beta_a) && al16(mean_a) && al16(var_a) && al16(xb) && al16(gamma_b) && al16(beta_b) &&
                    al16(mean_b) && al16(var_b) && al16(y), "bn_infer_fwd_pair: pointers must be 16-byte aligned")) return e;
    if (int e = chk(y != xa && y != xb, "bn_infer_fwd_pair: y must be a buffer of its own")) return e;
    const size_t n4 = (size_t)P * C / 4;
    hipLaunchKernelGGL(k_bn_infer_pair, dim3(ew_grid(n4)), dim3(NT), 0, (hipStream_t)stream, xa, gamma_a, beta_a, mean_a, var_a, xb, gamma_b,
                       beta_b, mean_b, var_b, y, n4, C / 4, eps);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_bn_frozen_bwd_pair_f32(const float *gy, const float *y, const float *gamma_a, const float *var_a, const float *gamma_b,
                                            const float *var_b, float *gxa, float *gxb, int P, int C, float eps, void *stream) {
    if (int e = chk(gy && gamma_a && var_a && gamma_b && var_b && gxa && gxb, "bn_frozen_bwd_pair: null pointer")) return e;
    if (int e = chk(P > 0 && C > 0 && (C % 4) == 0, "bn_frozen_bwd_pair: need P>0, C%4==0")) return e;
    if (int e = chk(al16(gy) && al16(y) && al16(gamma_a) && al16(var_a) && al16(gamma_b) && al16(var_b) && al16(gxa) && al16(gxb),
                    "bn_frozen_bwd_pair: pointers must be 16-byte aligned")) return e;
    if (int e = chk(gxa != gxb, "bn_frozen_bwd_pair: gxa and gxb must be different buffers")) return e;
    const size_t n4 = (size_t)P * C / 4;
    hipLaunchKernelGGL(k_bn_frozen_bwd_pair, dim3(ew_grid(n4)), dim3(NT), 0, (hipStream_t)stream, gy, y, gamma_a, var_a, gamma_b, var_b, gxa,
                       gxb, n4, C / 4, eps);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_sgd_momentum_wd_masked_f32(float *p, const float *g, float *v, size_t n, size_t offset, const uint32_t *frozen_blocks,
                                                size_t n_blocks, float lr, float momentum, float weight_decay, void *stream) {
    if (n == 0) return 0;
    if (int e = chk(p && g && v && frozen_blocks, "sgd_momentum_wd_masked: null pointer")) return e;
    if (int e = chk(offset + n >= n && (offset + n + 63) / 64 <= n_blocks, "sgd_momentum_wd_masked: [offset, offset + n) lies outside the n_blocks x 64 floats the mask covers")) return e;
    // the float4 groups are those of the flat buffer: the section's pointers must sit at 4 * (offset % 4) bytes past a 16-byte boundary
    const uintptr_t want = (offset & 3) * sizeof(float);
    if (int e = chk(((uintptr_t)p & 15) == want && ((uintptr_t)g & 15) == want && ((uintptr_t)v & 15) == want && ((uintptr_t)frozen_blocks & 3) == 0,
                    "sgd_momentum_wd_masked: p / g / v must be element `offset` of 16-byte aligned flat buffers, the mask 4-byte aligned")) return e;
    hipLaunchKernelGGL(k_sgd_masked, dim3(ew_grid(std::max<size_t>(n / 4, 1))), dim3(NT), 0, (hipStream_t)stream, p, g, v, n, offset,
                       frozen_blocks, lr, momentum, weight_decay);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
