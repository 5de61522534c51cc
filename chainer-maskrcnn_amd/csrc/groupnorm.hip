// GroupNorm of the RoI heads (nn/core.py GroupNorm; the arithmetic is gn_common.h).  NHWC float32 (R, H, W, Cp), C logical
// channels in G groups of cpg = C / G, statistics per (sample, group) over n = H * W * cpg elements, variance about the mean.
//   k_gn_fwd_reg / k_gn_bwd_reg   path 0.  A 256-thread workgroup owns one (sample, slab): `cols` float4 columns of every pixel - 8 columns
//       (32 channels, 128 contiguous bytes per pixel) where cpg divides 32, else the cpg / 4 columns of one group.  Thread t = (row t / cols,
//       column t % cols) holds pixels row, row + rows, ... (rows = 256 / cols, at most NI of them) in registers: x (and gy) come from
//       memory exactly once.  A float4 may straddle 4 (cpg 1) or 2 (cpg 2) groups: sums are kept per member and reduced per channel first
//       (slab_reduce: xor shuffles over the lanes of a column where cols is a power of two, then one LDS step over the waves, in a
//       fixed order), then per group from the channel sums.
//   k_gn_fwd_gen / k_gn_bwd_gen   path 1: any cpg, any H * W.  One workgroup per (sample, group) walks its elements three times (sum, squared
//       deviations, apply) / per channel and then once more (sums, apply); one more workgroup per sample zero-fills the padded channels.
//   k_gn_param_reduce             ggamma / gbeta: the backward kernels leave one partial row per sample in the caller's workspace
//       (2, R, Cp); this sums them over R in a fixed order.  No float atomics anywhere: the same input gives the same bits.
// Every access is guarded by p < H * W and c < Cp; padded channels (c >= C) of y and gx are written as exact zeros.
#include "gn_common.h"

namespace {

constexpr int NT = 256;
constexpr int NI_MAX = 8;          // pixels a thread of the register path holds: 8 float4 of x, and 8 of gy in the backward
constexpr int COLS_MAX = 64;       // float4 columns of a slab (one wave wide)
constexpr int GPS_MAX = 32;        // groups of a slab (cpg 1 on 8 columns)

struct Geom {
    int path, cols, rows, pow2, gps, slabs, ni;
};

// the launch geometry of a valid (H * W, Cp, cpg); host arithmetic
Geom geom_of(long long HW, int Cp, int cpg) {
    Geom g = {1, 0, 0, 0, 0, 0, 0};
    if (!(cpg == 1 || cpg == 2 || cpg % 4 == 0)) return g;
    const int cols = (32 % cpg == 0) ? 8 : cpg / 4;
    if (cols > COLS_MAX) return g;
    const int rows = NT / cols;
    if (HW > (long long)rows * NI_MAX) return g;
    g.path = 0;
    g.cols = cols;
    g.rows = rows;
    g.pow2 = (cols & (cols - 1)) == 0;
    g.gps = cols * 4 / cpg;
    g.slabs = (Cp + cols * 4 - 1) / (cols * 4);
    const int need = (int)((HW + rows - 1) / rows);
    g.ni = need <= 2 ? 2 : (need <= 4 ? 4 : NI_MAX);
    return g;
}

// Sums the members of v[0..NQ) over the threads of the workgroup that share a column: chs[k * 256 + j] = sum of quantity k over channel j
// of the slab (j < cols * 4), visible to every thread on return.  part: NQ * 1024 floats, chs: NQ * 256 floats of LDS.  Fixed order.
template <int NQ>
__device__ __forceinline__ void slab_reduce(float4 (&v)[NQ], int cols, int rows, int pow2, int q, int p0, float *__restrict__ part,
                                            float *__restrict__ chs) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    int slot, nslots;
    bool writer;
    if (pow2) {                                              // lanes of a column are cols apart: cols divides the wave
        for (int off = cols; off < kWave; off <<= 1)
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                v[k].x += __shfl_xor(v[k].x, off, kWave); v[k].y += __shfl_xor(v[k].y, off, kWave);
                v[k].z += __shfl_xor(v[k].z, off, kWave); v[k].w += __shfl_xor(v[k].w, off, kWave);
            }
        slot = wave; nslots = NT / kWave; writer = lane < cols;
    } else {
        slot = p0; nslots = rows; writer = p0 < rows;
    }
    __syncthreads();                                         // (what an earlier reduction left in part / chs has been read)
    if (writer)
#pragma unroll
        for (int k = 0; k < NQ; ++k) *reinterpret_cast<float4 *>(part + k * 1024 + (slot * cols + q) * 4) = v[k];
    __syncthreads();
    const int j = threadIdx.x;
    if (j < cols * 4)
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            float s = 0.f;
            for (int sl = 0; sl < nslots; ++sl) s += part[k * 1024 + sl * cols * 4 + j];
            chs[k * 256 + j] = s;
        }
    __syncthreads();
}

__device__ __forceinline__ float4 pick4(const float *__restrict__ tab, const int (&gl)[4]) {
    return make_float4(tab[gl[0]], tab[gl[1]], tab[gl[2]], tab[gl[3]]);
}

// grid R * slabs
template <int NI>
__global__ __launch_bounds__(NT) void k_gn_fwd_reg(const float *__restrict__ x, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, float *__restrict__ y, float *__restrict__ mean,
                                                   float *__restrict__ rstd, int HW, int C, int Cp, int G, int cpg, int cols, int rows,
                                                   int pow2, int gps, int slabs, float eps, int relu, float n) {
    __shared__ __attribute__((aligned(16))) float part[1024];
    __shared__ float chs[256];
    __shared__ float g_mean[GPS_MAX], g_rstd[GPS_MAX];
    const int r = blockIdx.x / slabs, slab = blockIdx.x - r * slabs;
    const int t = threadIdx.x, q = t % cols, p0 = t / cols;
    const int c0 = slab * cols * 4 + q * 4;
    const bool active = p0 < rows && c0 < Cp;
    unsigned keep = 0u;
    int gl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (active && c0 + k < C) keep |= 1u << k;
        gl[k] = (q * 4 + k) / cpg;                           // < gps
    }
    const size_t base = (size_t)r * HW * Cp + c0;
    float4 xv[NI];
    float4 s[1] = {f4(0.f)};
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = p0 + rows * i;
        xv[i] = (active && p < HW) ? gn_keep4(ld4(x + base + (size_t)p * Cp), keep) : f4(0.f);
        s[0] = add4(s[0], xv[i]);
    }
    slab_reduce<1>(s, cols, rows, pow2, q, p0, part, chs);
    if (t < gps) {
        float a = 0.f;
        for (int i = 0; i < cpg; ++i) a += chs[t * cpg + i];
        g_mean[t] = a / n;
    }
    __syncthreads();
    const float4 m4 = pick4(g_mean, gl);
    s[0] = f4(0.f);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = p0 + rows * i;
        if (active && p < HW) {
            float4 d; d.x = xv[i].x - m4.x; d.y = xv[i].y - m4.y; d.z = xv[i].z - m4.z; d.w = xv[i].w - m4.w;
            s[0] = add4(s[0], gn_keep4(mul4(d, d), keep));
        }
    }
    slab_reduce<1>(s, cols, rows, pow2, q, p0, part, chs);
    if (t < gps) {
        float a = 0.f;
        for (int i = 0; i < cpg; ++i) a += chs[t * cpg + i];
        const float rs = gn_rstd1(a / n, eps);
        g_rstd[t] = rs;
        const int g = slab * gps + t;
        if (g < G) {
            if (mean) mean[(size_t)r * G + g] = g_mean[t];
            if (rstd) rstd[(size_t)r * G + g] = rs;
        }
    }
    __syncthreads();
    if (!active) return;
    const float4 s4 = pick4(g_rstd, gl);
    const float4 ga = ld4(gamma + c0), be = ld4(beta + c0);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = p0 + rows * i;
        if (p < HW) {
            float4 o = gn_affine4(xv[i], ga, m4, s4, be);
            if (relu) o = relu4(o);
            st4(y + base + (size_t)p * Cp, gn_keep4(o, keep));
        }
    }
}

// grid R * slabs.  ws (2, R, Cp): row r of plane 0 = sum over the pixels of gy, of plane 1 = sum of gy * xhat, per channel (0 on padding)
template <int NI>
__global__ __launch_bounds__(NT) void k_gn_bwd_reg(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, const float *__restrict__ mean,
                                                   const float *__restrict__ rstd, float *__restrict__ gx, float *__restrict__ ws, int R,
                                                   int HW, int C, int Cp, int G, int cpg, int cols, int rows, int pow2, int gps, int slabs,
                                                   int relu, float n) {
    __shared__ __attribute__((aligned(16))) float part[2 * 1024];
    __shared__ float chs[2 * 256];
    __shared__ float g_a[GPS_MAX], g_b[GPS_MAX];
    const int r = blockIdx.x / slabs, slab = blockIdx.x - r * slabs;
    const int t = threadIdx.x, q = t % cols, p0 = t / cols;
    const int c0 = slab * cols * 4 + q * 4;
    const bool active = p0 < rows && c0 < Cp;
    unsigned keep = 0u;
    float4 m4 = f4(0.f), s4 = f4(0.f);
    {
        float mm[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (active && c0 + k < C) {
                keep |= 1u << k;
                const int g = (c0 + k) / cpg;                // < G
                mm[k] = mean[(size_t)r * G + g];
                ss[k] = rstd[(size_t)r * G + g];
            }
        m4 = make_float4(mm[0], mm[1], mm[2], mm[3]);
        s4 = make_float4(ss[0], ss[1], ss[2], ss[3]);
    }
    const float4 ga = active ? gn_keep4(ld4(gamma + c0), keep) : f4(0.f);
    const float4 be = active ? ld4(beta + c0) : f4(0.f);
    const size_t base = (size_t)r * HW * Cp + c0;
    float4 gv[NI], xh[NI];
    float4 s[2] = {f4(0.f), f4(0.f)};
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = p0 + rows * i;
        gv[i] = xh[i] = f4(0.f);
        if (active && p < HW) {
            const float4 xv = ld4(x + base + (size_t)p * Cp);
            float4 g = ld4(gy + base + (size_t)p * Cp);
            if (relu) g = relu_mask4(g, gn_affine4(xv, ga, m4, s4, be));
            gv[i] = gn_keep4(g, keep);
            xh[i] = gn_keep4(gn_xhat4(xv, m4, s4), keep);
            s[0] = add4(s[0], gv[i]);
            s[1] = gn_dot4(gv[i], xh[i], s[1]);
        }
    }
    slab_reduce<2>(s, cols, rows, pow2, q, p0, part, chs);
    if (t < cols * 4) {
        const int c = slab * cols * 4 + t;
        if (c < Cp) {
            ws[(size_t)r * Cp + c] = chs[t];
            ws[((size_t)R + r) * Cp + c] = chs[256 + t];
        }
    }
    if (t < gps) {
        float a = 0.f, b = 0.f;
        for (int i = 0; i < cpg; ++i) {
            const int c = slab * cols * 4 + t * cpg + i;
            const float gm = c < C ? gamma[c] : 0.f;
            a += gm * chs[t * cpg + i];
            b += gm * chs[256 + t * cpg + i];
        }
        g_a[t] = a / n;
        g_b[t] = b / n;
    }
    __syncthreads();
    if (!active) return;
    int gl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gl[k] = (q * 4 + k) / cpg;
    const float4 a4 = pick4(g_a, gl), b4 = pick4(g_b, gl);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = p0 + rows * i;
        if (p < HW) st4(gx + base + (size_t)p * Cp, gn_keep4(gn_bwd_dx4(gv[i], xh[i], ga, s4, a4, b4), keep));
    }
}

// sum of a and of b over the workgroup, in every thread; sh: 2 * NT / kWave floats.  Fixed order.
__device__ __forceinline__ void block_sum2(float &a, float &b, float *__restrict__ sh) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, kWave);
        b += __shfl_xor(b, off, kWave);
    }
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    __syncthreads();                                         // (the previous sums have been read)
    if (lane == 0) {
        sh[2 * wave] = a;
        sh[2 * wave + 1] = b;
    }
    __syncthreads();
    a = b = 0.f;
#pragma unroll
    for (int w = 0; w < NT / kWave; ++w) {
        a += sh[2 * w];
        b += sh[2 * w + 1];
    }
}

// the padded channels [C, Cp) of sample r of t (R, HW, Cp) as zeros
__device__ __forceinline__ void zero_padding(float *__restrict__ t, int r, int HW, int C, int Cp) {
    const int np = Cp - C;
    for (long long e = threadIdx.x; e < (long long)HW * np; e += NT) {
        const long long p = e / np;
        t[((size_t)r * HW + p) * Cp + C + (int)(e - p * np)] = 0.f;
    }
}

// grid R * (G + 1): workgroup (r, g < G) normalises group g of sample r; (r, G) zero-fills the padded channels
__global__ __launch_bounds__(NT) void k_gn_fwd_gen(const float *__restrict__ x, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, float *__restrict__ y, float *__restrict__ mean,
                                                   float *__restrict__ rstd, int HW, int C, int Cp, int G, int cpg, float eps, int relu,
                                                   float n) {
    __shared__ float sh[2 * NT / kWave];
    const int r = blockIdx.x / (G + 1), g = blockIdx.x - r * (G + 1);
    if (g == G) {
        zero_padding(y, r, HW, C, Cp);
        return;
    }
    const long long ne = (long long)HW * cpg;
    const size_t base = (size_t)r * HW * Cp + (size_t)g * cpg;
    float a = 0.f, b = 0.f;
    for (long long e = threadIdx.x; e < ne; e += NT) {
        const long long p = e / cpg;
        a += x[base + (size_t)p * Cp + (int)(e - p * cpg)];
    }
    block_sum2(a, b, sh);
    const float m = a / n;
    a = b = 0.f;
    for (long long e = threadIdx.x; e < ne; e += NT) {
        const long long p = e / cpg;
        const float d = x[base + (size_t)p * Cp + (int)(e - p * cpg)] - m;
        a += d * d;
    }
    block_sum2(a, b, sh);
    const float rs = gn_rstd1(a / n, eps);
    if (threadIdx.x == 0) {
        if (mean) mean[(size_t)r * G + g] = m;
        if (rstd) rstd[(size_t)r * G + g] = rs;
    }
    for (long long e = threadIdx.x; e < ne; e += NT) {
        const long long p = e / cpg;
        const int j = (int)(e - p * cpg), c = g * cpg + j;
        const float o = gn_affine1(x[base + (size_t)p * Cp + j], gamma[c], m, rs, beta[c]);
        y[base + (size_t)p * Cp + j] = relu ? relu1(o) : o;
    }
}

// grid R * (G + 1), as the forward; ws as in k_gn_bwd_reg
__global__ __launch_bounds__(NT) void k_gn_bwd_gen(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, const float *__restrict__ mean,
                                                   const float *__restrict__ rstd, float *__restrict__ gx, float *__restrict__ ws, int R,
                                                   int HW, int C, int Cp, int G, int cpg, int relu, float n) {
    __shared__ float sh[2 * NT / kWave];
    const int r = blockIdx.x / (G + 1), g = blockIdx.x - r * (G + 1);
    if (g == G) {
        zero_padding(gx, r, HW, C, Cp);
        for (int c = C + threadIdx.x; c < Cp; c += NT) {
            ws[(size_t)r * Cp + c] = 0.f;
            ws[((size_t)R + r) * Cp + c] = 0.f;
        }
        return;
    }
    const float m = mean[(size_t)r * G + g], rs = rstd[(size_t)r * G + g];
    const size_t base = (size_t)r * HW * Cp + (size_t)g * cpg;
    float A = 0.f, B = 0.f;
    for (int j = 0; j < cpg; ++j) {
        const int c = g * cpg + j;
        const float ga = gamma[c], be = beta[c];
        float a = 0.f, b = 0.f;
        for (int p = threadIdx.x; p < HW; p += NT) {
            const float xv = x[base + (size_t)p * Cp + j];
            float gv = gy[base + (size_t)p * Cp + j];
            if (relu) gv = relu_mask1(gv, gn_affine1(xv, ga, m, rs, be));
            a += gv;
            b = gn_dot1(gv, gn_xhat1(xv, m, rs), b);
        }
        block_sum2(a, b, sh);
        if (threadIdx.x == 0) {
            ws[(size_t)r * Cp + c] = a;
            ws[((size_t)R + r) * Cp + c] = b;
        }
        A += ga * a;
        B += ga * b;
    }
    A = A / n;
    B = B / n;
    const long long ne = (long long)HW * cpg;
    for (long long e = threadIdx.x; e < ne; e += NT) {
        const long long p = e / cpg;
        const int j = (int)(e - p * cpg), c = g * cpg + j;
        const float ga = gamma[c];
        const float xv = x[base + (size_t)p * Cp + j];
        float gv = gy[base + (size_t)p * Cp + j];
        if (relu) gv = relu_mask1(gv, gn_affine1(xv, ga, m, rs, beta[c]));
        gx[base + (size_t)p * Cp + j] = gn_bwd_dx1(gv, gn_xhat1(xv, m, rs), ga, rs, A, B);
    }
}

// grid (cdiv(Cp, 32), 2): plane blockIdx.y of ws (2, R, Cp) summed over R into gbeta (plane 0) / ggamma (plane 1), 32 channels per workgroup
__global__ __launch_bounds__(NT) void k_gn_param_reduce(const float *__restrict__ ws, float *__restrict__ ggamma, float *__restrict__ gbeta,
                                                        int R, int Cp, int accumulate) {
    __shared__ __attribute__((aligned(16))) float part[1024];
    __shared__ float chs[256];
    const int t = threadIdx.x, q = t % 8, p0 = t / 8;
    const int c0 = blockIdx.x * 32 + q * 4;
    const float *plane = ws + (size_t)blockIdx.y * R * Cp;
    float4 s[1] = {f4(0.f)};
    if (c0 < Cp)
        for (int r = p0; r < R; r += NT / 8) s[0] = add4(s[0], ld4(plane + (size_t)r * Cp + c0));
    slab_reduce<1>(s, 8, NT / 8, 1, q, p0, part, chs);
    const int c = blockIdx.x * 32 + t;
    if (t < 32 && c < Cp) {
        float *out = blockIdx.y ? ggamma : gbeta;
        out[c] = accumulate ? out[c] + chs[t] : chs[t];
    }
}

inline bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// the checks the plan query and both entry points share; cpg and H * W on success
int check_geometry(const char *who, int R, int H, int W, int C, int Cp, int G) {
    if (R < 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: R = %d is negative", who, R);
    if (H <= 0 || W <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad size H x W = %d x %d", who, H, W);
    if (C <= 0 || G <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: C = %d, G = %d must be positive", who, C, G);
    if (C % G != 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: G = %d does not divide C = %d", who, G, C);
    if (Cp < C) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: Cp = %d is below C = %d", who, Cp, C);
    if (Cp % 4 != 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: Cp = %d is not a multiple of 4", who, Cp);
    if ((long long)H * W > 0x7FFFFFFFLL || (long long)H * W * Cp > 0x7FFFFFFFLL) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: H * W * Cp = %d * %d * %d exceeds int32", who, H, W, Cp);
    const Geom g = geom_of((long long)H * W, Cp, C / G);
    const long long blocks = (long long)R * (g.path == 0 ? g.slabs : G + 1);
    if (blocks > 0x7FFFFFFFLL) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: R = %d needs more than 2^31 workgroups", who, R);
    return 0;
}

size_t bwd_ws_bytes_of(int R, int Cp) { return (size_t)2 * R * Cp * sizeof(float); }

}  // namespace

extern "C" int mrcnn_group_norm_plan(int R, int H, int W, int C, int Cp, int G, int *path, size_t *bwd_ws_bytes) {
    if (int e = check_geometry("group_norm_plan", R, H, W, C, Cp, G)) return e;
    if (path) *path = geom_of((long long)H * W, Cp, C / G).path;
    if (bwd_ws_bytes) *bwd_ws_bytes = bwd_ws_bytes_of(R, Cp);
    return 0;
}

extern "C" int mrcnn_group_norm_fwd_f32(const float *x, const float *gamma, const float *beta, int R, int H, int W, int C, int Cp, int G,
                                        float eps, int relu, float *y, float *mean, float *rstd, void *stream) {
    const char *who = "group_norm_fwd";
    if (int e = check_geometry(who, R, H, W, C, Cp, G)) return e;
    if (!(eps > 0.f)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: eps must be positive", who);
    if (relu != 0 && relu != 1) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: relu = %d outside 0..1", who, relu);
    if (R == 0) return 0;
    if (!x) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null x", who);
    if (!gamma) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gamma", who);
    if (!beta) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null beta", who);
    if (!y) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null y", who);
    if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(y))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: x, gamma, beta and y must be 16-byte aligned", who);
    const int HW = H * W, cpg = C / G;
    const float n = (float)((long long)HW * cpg);
    const Geom g = geom_of(HW, Cp, cpg);
    hipStream_t st = (hipStream_t)stream;
    if (g.path == 0) {
        const dim3 grid((unsigned)(R * g.slabs));
#define GN_FWD(NI)                                                                                                                      \
    hipLaunchKernelGGL(k_gn_fwd_reg<NI>, grid, dim3(NT), 0, st, x, gamma, beta, y, mean, rstd, HW, C, Cp, G, cpg, g.cols, g.rows, g.pow2, \
                       g.gps, g.slabs, eps, relu, n)
        if (g.ni == 2) GN_FWD(2);
        else if (g.ni == 4) GN_FWD(4);
        else GN_FWD(NI_MAX);
#undef GN_FWD
    } else {
        hipLaunchKernelGGL(k_gn_fwd_gen, dim3((unsigned)(R * (G + 1))), dim3(NT), 0, st, x, gamma, beta, y, mean, rstd, HW, C, Cp, G, cpg, eps,
                           relu, n);
    }
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_group_norm_bwd_f32(const float *gy, const float *x, const float *gamma, const float *beta, const float *mean,
                                        const float *rstd, int R, int H, int W, int C, int Cp, int G, int relu, float *gx, float *ggamma,
                                        float *gbeta, int accumulate_params, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "group_norm_bwd";
    if (int e = check_geometry(who, R, H, W, C, Cp, G)) return e;
    if (relu != 0 && relu != 1) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: relu = %d outside 0..1", who, relu);
    if (R == 0) return 0;                                     // (no sample: the parameter gradients are left as they are)
    if (!gy) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gy", who);
    if (!x) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null x", who);
    if (!gamma) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gamma", who);
    if (!beta) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null beta", who);
    if (!mean) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null mean", who);
    if (!rstd) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null rstd", who);
    if (!gx) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gx", who);
    if (!ggamma) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null ggamma", who);
    if (!gbeta) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gbeta", who);
    if (!ws) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null workspace", who);
    if (ws_bytes < bwd_ws_bytes_of(R, Cp))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, bwd_ws_bytes_of(R, Cp));
    if (!aligned16(gy) || !aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(gx) || !aligned16(ggamma) ||
        !aligned16(gbeta) || !aligned16(ws))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: gy, x, gamma, beta, gx, ggamma, gbeta and the workspace must be 16-byte aligned", who);
    const int HW = H * W, cpg = C / G;
    const float n = (float)((long long)HW * cpg);
    const Geom g = geom_of(HW, Cp, cpg);
    hipStream_t st = (hipStream_t)stream;
    float *wsf = static_cast<float *>(ws);
    if (g.path == 0) {
        const dim3 grid((unsigned)(R * g.slabs));
#define GN_BWD(NI)                                                                                                                       \
    hipLaunchKernelGGL(k_gn_bwd_reg<NI>, grid, dim3(NT), 0, st, gy, x, gamma, beta, mean, rstd, gx, wsf, R, HW, C, Cp, G, cpg, g.cols, g.rows, \
                       g.pow2, g.gps, g.slabs, relu, n)
        if (g.ni == 2) GN_BWD(2);
        else if (g.ni == 4) GN_BWD(4);
        else GN_BWD(NI_MAX);
#undef GN_BWD
    } else {
        hipLaunchKernelGGL(k_gn_bwd_gen, dim3((unsigned)(R * (G + 1))), dim3(NT), 0, st, gy, x, gamma, beta, mean, rstd, gx, wsf, R, HW, C, Cp, G,
                           cpg, relu, n);
    }
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gn_param_reduce, dim3(mrcnn::cdiv(Cp, 32), 2), dim3(NT), 0, st, wsf, ggamma, gbeta, R, Cp, accumulate_params);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
