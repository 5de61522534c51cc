// GroupNorm of whole feature maps (nn/core.py MapGroupNorm: the FPN's convolutions; the arithmetic is gn_common.h).  NHWC
// float32 (R, H, W, Cp), C logical channels in G groups of cpg = C / G, cpg a multiple of 4 (a float4 never leaves its group), Cp <= 1024.
// A (sample, group) is split over many workgroups: a CHUNK is a contiguous pixel range of one sample, pixels_per_chunk a function of
// (H * W, Cp) alone, and a 256-thread workgroup owns one (sample, chunk) over all channels.  Thread t = (row t / cols, column t % cols),
// cols = Cp / 4, rows = 256 / cols, keeps its float4 column and walks the pixels row, row + rows, ... of the chunk with its sums in
// registers; chunk_reduce sums them over the rows in LDS in a fixed order, then one thread per group sums its channels.
//   forward   k_gnm_stats     per (sample, chunk) and group: the chunk's own mean, then M2 about it in a second sweep (the chunk is L2-resident)
//             k_gnm_merge     per (sample, group): gn_merge1 over the chunks in index order -> mean, rstd
//             k_gnm_apply     y = gn_affine(x)
//   backward  k_gnm_bwd_sums  per (sample, chunk) and channel: sum gy, sum gy * xhat -> partial rows (2, R * chunks, Cp)
//             k_gnm_bwd_final per (sample, channel) the rows summed over the chunks in index order; per (sample, group) the two means the
//                             data gradient needs; ggamma / gbeta summed over the samples in index order
//             k_gnm_bwd_dx    gx = gn_bwd_dx(...)
// Every hand-over between workgroups is a kernel boundary: no atomics, no counters, no grid barrier - the same input gives the same bits.
// Every access is guarded by p < chunk end and c < Cp; padded channels (c >= C) of y and gx are written as exact zeros.
#include "gn_common.h"

namespace {

constexpr int NT = 256;
constexpr int CP_MAX = 1024;       // cols = Cp / 4 float4 columns fit one workgroup
constexpr int CPG_MAX = 256;
constexpr int CHUNKS_TARGET = 256; // chunks of a sample: two workgroups for each of the 256 CUs at the two images of a training batch
constexpr int PPT_MIN = 8;         // pixels a thread walks in the smallest chunk
constexpr int PPT_MAX = 256;       // and in the largest: 1024 pixels (1 MiB) at Cp 256
constexpr int LOADS = 16;          // workspace rows a thread of the merge / finalize kernels loads before it folds them

struct MapGeom {
    int cols, rows, ppc, chunks;
};

// The launch geometry of a valid (H * W, Cp); host arithmetic.  Deliberately not a function of R: the chunks of a sample, and with them the
// summation tree of its statistics, are the same whatever batch it arrives in, and the workspace is linear in R.
MapGeom map_geom(long long HW, int Cp) {
    MapGeom g;
    g.cols = Cp / 4;
    g.rows = NT / g.cols;
    const long long step = 4LL * g.rows;                     // (whole trips of the unrolled sweep)
    long long ppc = (HW + CHUNKS_TARGET - 1) / CHUNKS_TARGET;
    ppc = (ppc + step - 1) / step * step;
    if (ppc < (long long)PPT_MIN * g.rows) ppc = (long long)PPT_MIN * g.rows;
    if (ppc > (long long)PPT_MAX * g.rows) ppc = (long long)PPT_MAX * g.rows;
    g.ppc = (int)ppc;
    g.chunks = (int)((HW + ppc - 1) / ppc);
    return g;
}

// Sums v[0..NQ) over the threads of the workgroup that share a column: chs[k * CP_MAX + c] = sum of quantity k over channel c < Cp, visible
// to every thread on return.  part: NQ * 1024 floats, chs: NQ * CP_MAX floats of LDS.  Fixed order.
template <int NQ>
__device__ __forceinline__ void chunk_reduce(const float4 (&v)[NQ], int Cp, int cols, int rows, int q, int p0, float *__restrict__ part,
                                             float *__restrict__ chs) {
    __syncthreads();                                         // (what an earlier reduction left in part / chs has been read)
    if (p0 < rows)
#pragma unroll
        for (int k = 0; k < NQ; ++k) *reinterpret_cast<float4 *>(part + k * 1024 + (p0 * cols + q) * 4) = v[k];
    __syncthreads();
    for (int c = threadIdx.x; c < Cp; c += NT)
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            float s = 0.f;
            for (int row = 0; row < rows; ++row) s += part[k * 1024 + row * Cp + c];
            chs[k * CP_MAX + c] = s;
        }
    __syncthreads();
}

struct Chunk {
    int r, p_begin, p_end, q, p0, c0;
    bool walks, live;              // walks: the thread owns a column of the chunk; live: that column holds logical channels
};

__device__ __forceinline__ Chunk chunk_of(int HW, int C, int cols, int rows, int ppc, int chunks) {
    Chunk k;
    k.r = blockIdx.x / chunks;
    const int ch = blockIdx.x - k.r * chunks;
    k.p_begin = ch * ppc;
    k.p_end = min(HW, k.p_begin + ppc);
    k.q = threadIdx.x % cols;
    k.p0 = threadIdx.x / cols;
    k.c0 = k.q * 4;
    k.walks = k.p0 < rows;
    k.live = k.walks && k.c0 < C;                            // (C is a multiple of 4: a float4 is logical or padding as a whole)
    return k;
}

// grid R * chunks.  ws_mean / ws_m2 (R * chunks, G)
__global__ __launch_bounds__(NT) void k_gnm_stats(const float *__restrict__ x, float *__restrict__ ws_mean, float *__restrict__ ws_m2, int HW,
                                                  int C, int Cp, int G, int cpg, int cols, int rows, int ppc, int chunks) {
    __shared__ __attribute__((aligned(16))) float part[1024];
    __shared__ float chs[CP_MAX];
    __shared__ float g_mean[CP_MAX / 4];
    const Chunk k = chunk_of(HW, C, cols, rows, ppc, chunks);
    const int t = threadIdx.x;
    const float cnt = (float)((k.p_end - k.p_begin) * cpg);
    const float *xb = x + (size_t)k.r * HW * Cp + k.c0;
    const size_t st = (size_t)rows * Cp;
    float4 s[1] = {f4(0.f)};
    if (k.live) {
        int p = k.p_begin + k.p0;
        for (; p + 3 * rows < k.p_end; p += 4 * rows) {
            const float *a = xb + (size_t)p * Cp;
            const float4 v0 = ld4(a), v1 = ld4(a + st), v2 = ld4(a + 2 * st), v3 = ld4(a + 3 * st);
            s[0] = add4(add4(add4(add4(s[0], v0), v1), v2), v3);
        }
        for (; p < k.p_end; p += rows) s[0] = add4(s[0], ld4(xb + (size_t)p * Cp));
    }
    chunk_reduce<1>(s, Cp, cols, rows, k.q, k.p0, part, chs);
    if (t < G) {
        float a = 0.f;
        for (int i = 0; i < cpg; ++i) a += chs[t * cpg + i];
        g_mean[t] = a / cnt;
    }
    __syncthreads();
    s[0] = f4(0.f);
    if (k.live) {
        const float4 m4 = f4(g_mean[k.c0 / cpg]);
        int p = k.p_begin + k.p0;
        for (; p + 3 * rows < k.p_end; p += 4 * rows) {
            const float *a = xb + (size_t)p * Cp;
            const float4 v0 = ld4(a), v1 = ld4(a + st), v2 = ld4(a + 2 * st), v3 = ld4(a + 3 * st);
            s[0] = add4(add4(add4(add4(s[0], gn_sqdev4(v0, m4)), gn_sqdev4(v1, m4)), gn_sqdev4(v2, m4)), gn_sqdev4(v3, m4));
        }
        for (; p < k.p_end; p += rows) s[0] = add4(s[0], gn_sqdev4(ld4(xb + (size_t)p * Cp), m4));
    }
    chunk_reduce<1>(s, Cp, cols, rows, k.q, k.p0, part, chs);
    if (t < G) {
        float a = 0.f;
        for (int i = 0; i < cpg; ++i) a += chs[t * cpg + i];
        ws_mean[(size_t)blockIdx.x * G + t] = g_mean[t];
        ws_m2[(size_t)blockIdx.x * G + t] = a;
    }
}

// one thread per (sample, group).  st_mean / st_rstd (R, G): the workspace's copy the apply kernel reads; mean / rstd: the caller's, nullable
__global__ __launch_bounds__(NT) void k_gnm_merge(const float *__restrict__ ws_mean, const float *__restrict__ ws_m2, float *__restrict__ st_mean,
                                                  float *__restrict__ st_rstd, float *__restrict__ mean, float *__restrict__ rstd, int R, int HW,
                                                  int G, int cpg, int ppc, int chunks, float eps, float n_all) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= R * G) return;
    const int r = e / G, g = e - r * G;
    const size_t row0 = (size_t)r * chunks;
    float n = (float)(min(HW, ppc) * cpg), m = ws_mean[row0 * G + g], M2 = ws_m2[row0 * G + g];
    // the merge is one dependent chain: the loads of LOADS chunks are issued together (the index clamped, so none is conditional), then
    // folded in index order - a load's latency is paid once per batch, not once per chunk
    for (int i0 = 1; i0 < chunks; i0 += LOADS) {
        float mi[LOADS], qi[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const int i = min(i0 + j, chunks - 1);
            mi[j] = ws_mean[(row0 + i) * G + g];
            qi[j] = ws_m2[(row0 + i) * G + g];
        }
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const int i = i0 + j;
            if (i < chunks) gn_merge1(n, m, M2, (float)((min(HW, (i + 1) * ppc) - i * ppc) * cpg), mi[j], qi[j]);
        }
    }
    const float rs = gn_rstd1(M2 / n_all, eps);
    st_mean[e] = m;
    st_rstd[e] = rs;
    if (mean) mean[e] = m;
    if (rstd) rstd[e] = rs;
}

// grid R * chunks
__global__ __launch_bounds__(NT) void k_gnm_apply(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                  const float *__restrict__ st_mean, const float *__restrict__ st_rstd, float *__restrict__ y,
                                                  int HW, int C, int Cp, int G, int cpg, int cols, int rows, int ppc, int chunks) {
    const Chunk k = chunk_of(HW, C, cols, rows, ppc, chunks);
    if (!k.walks) return;
    const size_t base = (size_t)k.r * HW * Cp + k.c0;
    if (!k.live) {
        for (int p = k.p_begin + k.p0; p < k.p_end; p += rows) st4(y + base + (size_t)p * Cp, f4(0.f));
        return;
    }
    const int g = k.c0 / cpg;
    const float4 m4 = f4(st_mean[(size_t)k.r * G + g]), s4 = f4(st_rstd[(size_t)k.r * G + g]);
    const float4 ga = ld4(gamma + k.c0), be = ld4(beta + k.c0);
#pragma unroll 4
    for (int p = k.p_begin + k.p0; p < k.p_end; p += rows)
        st4(y + base + (size_t)p * Cp, gn_affine4(ld4(x + base + (size_t)p * Cp), ga, m4, s4, be));
}

// grid R * chunks.  ws1 / ws2 (R * chunks, Cp): per channel the chunk's sum of gy / of gy * xhat (0 on padding)
__global__ __launch_bounds__(NT) void k_gnm_bwd_sums(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ mean,
                                                     const float *__restrict__ rstd, float *__restrict__ ws1, float *__restrict__ ws2, int HW,
                                                     int C, int Cp, int G, int cpg, int cols, int rows, int ppc, int chunks) {
    __shared__ __attribute__((aligned(16))) float part[2 * 1024];
    __shared__ float chs[2 * CP_MAX];
    const Chunk k = chunk_of(HW, C, cols, rows, ppc, chunks);
    float4 s[2] = {f4(0.f), f4(0.f)};
    if (k.live) {
        const int g = k.c0 / cpg;
        const float4 m4 = f4(mean[(size_t)k.r * G + g]), s4 = f4(rstd[(size_t)k.r * G + g]);
        const size_t base = (size_t)k.r * HW * Cp + k.c0;
        const size_t st = (size_t)rows * Cp;
        int p = k.p_begin + k.p0;
        for (; p + rows < k.p_end; p += 2 * rows) {
            const size_t o = base + (size_t)p * Cp;
            const float4 x0 = ld4(x + o), x1 = ld4(x + o + st), g0 = ld4(gy + o), g1 = ld4(gy + o + st);
            s[0] = add4(add4(s[0], g0), g1);
            s[1] = gn_dot4(g1, gn_xhat4(x1, m4, s4), gn_dot4(g0, gn_xhat4(x0, m4, s4), s[1]));
        }
        for (; p < k.p_end; p += rows) {
            const size_t o = base + (size_t)p * Cp;
            const float4 g0 = ld4(gy + o);
            s[0] = add4(s[0], g0);
            s[1] = gn_dot4(g0, gn_xhat4(ld4(x + o), m4, s4), s[1]);
        }
    }
    chunk_reduce<2>(s, Cp, cols, rows, k.q, k.p0, part, chs);
    for (int c = threadIdx.x; c < Cp; c += NT) {
        ws1[(size_t)blockIdx.x * Cp + c] = chs[c];
        ws2[(size_t)blockIdx.x * Cp + c] = chs[CP_MAX + c];
    }
}

// grid cdiv(G, gpb), gpb = 256 / cpg groups (gpb * cpg channels, one per thread) per workgroup.  ws_a / ws_b (R, G): sum_c gamma_c S1_c / n and
// sum_c gamma_c S2_c / n of the (sample, group).  Workgroup 0 also gives the padded channels of ggamma / gbeta their zeros.
__global__ __launch_bounds__(NT) void k_gnm_bwd_final(const float *__restrict__ ws1, const float *__restrict__ ws2, const float *__restrict__ gamma,
                                                      float *__restrict__ ws_a, float *__restrict__ ws_b, float *__restrict__ ggamma,
                                                      float *__restrict__ gbeta, int R, int C, int Cp, int G, int cpg, int gpb, int chunks,
                                                      int accumulate, float n) {
    __shared__ float sh1[NT], sh2[NT];
    const int t = threadIdx.x;
    const int c = blockIdx.x * gpb * cpg + t;
    const bool valid = t < gpb * cpg && c < C;
    const float gm = valid ? gamma[c] : 0.f;
    float gg = 0.f, gb = 0.f;
    for (int r = 0; r < R; ++r) {
        float t1 = 0.f, t2 = 0.f;
        if (valid)
            for (int i0 = 0; i0 < chunks; i0 += LOADS) {      // (batched loads, summed in index order: see k_gnm_merge)
                float a[LOADS], b[LOADS];
#pragma unroll
                for (int j = 0; j < LOADS; ++j) {
                    const size_t o = ((size_t)r * chunks + min(i0 + j, chunks - 1)) * Cp + c;
                    a[j] = ws1[o];
                    b[j] = ws2[o];
                }
#pragma unroll
                for (int j = 0; j < LOADS; ++j)
                    if (i0 + j < chunks) {
                        t1 += a[j];
                        t2 += b[j];
                    }
            }
        __syncthreads();                                     // (the previous sample's products have been read)
        sh1[t] = gm * t1;
        sh2[t] = gm * t2;
        __syncthreads();
        const int g = blockIdx.x * gpb + t;
        if (t < gpb && g < G) {
            float a = 0.f, b = 0.f;
            for (int i = 0; i < cpg; ++i) {
                a += sh1[t * cpg + i];
                b += sh2[t * cpg + i];
            }
            ws_a[(size_t)r * G + g] = a / n;
            ws_b[(size_t)r * G + g] = b / n;
        }
        gb += t1;
        gg += t2;
    }
    if (valid) {
        ggamma[c] = accumulate ? ggamma[c] + gg : gg;
        gbeta[c] = accumulate ? gbeta[c] + gb : gb;
    }
    if (blockIdx.x == 0 && !accumulate)
        for (int cc = C + t; cc < Cp; cc += NT) {
            ggamma[cc] = 0.f;
            gbeta[cc] = 0.f;
        }
}

// grid R * chunks
__global__ __launch_bounds__(NT) void k_gnm_bwd_dx(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ gamma,
                                                   const float *__restrict__ mean, const float *__restrict__ rstd, const float *__restrict__ ws_a,
                                                   const float *__restrict__ ws_b, float *__restrict__ gx, int HW, int C, int Cp, int G, int cpg,
                                                   int cols, int rows, int ppc, int chunks) {
    const Chunk k = chunk_of(HW, C, cols, rows, ppc, chunks);
    if (!k.walks) return;
    const size_t base = (size_t)k.r * HW * Cp + k.c0;
    if (!k.live) {
        for (int p = k.p_begin + k.p0; p < k.p_end; p += rows) st4(gx + base + (size_t)p * Cp, f4(0.f));
        return;
    }
    const size_t rg = (size_t)k.r * G + k.c0 / cpg;
    const float4 m4 = f4(mean[rg]), s4 = f4(rstd[rg]), a4 = f4(ws_a[rg]), b4 = f4(ws_b[rg]);
    const float4 ga = ld4(gamma + k.c0);
#pragma unroll 4
    for (int p = k.p_begin + k.p0; p < k.p_end; p += rows) {
        const size_t o = base + (size_t)p * Cp;
        st4(gx + o, gn_bwd_dx4(ld4(gy + o), gn_xhat4(ld4(x + o), m4, s4), ga, s4, a4, b4));
    }
}

inline bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// the checks the plan query and both entry points share
int check_geometry(const char *who, int R, int H, int W, int C, int Cp, int G) {
    if (R < 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: R = %d is negative", who, R);
    if (H <= 0 || W <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad size H x W = %d x %d", who, H, W);
    if (C <= 0 || G <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: C = %d, G = %d must be positive", who, C, G);
    if (C % G != 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: G = %d does not divide C = %d", who, G, C);
    if (Cp < C) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: Cp = %d is below C = %d", who, Cp, C);
    if (Cp % 4 != 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: Cp = %d is not a multiple of 4", who, Cp);
    if (Cp > CP_MAX) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: Cp = %d is above the map path's %d", who, Cp, CP_MAX);
    const int cpg = C / G;
    if (cpg % 4 != 0 || cpg > CPG_MAX)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: C / G = %d is not a multiple of 4 up to %d (use group_norm_*)", who, cpg, CPG_MAX);
    if ((long long)H * W > 0x7FFFFFFFLL || (long long)H * W * Cp > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: H * W * Cp = %d * %d * %d exceeds int32", who, H, W, Cp);
    const MapGeom g = map_geom((long long)H * W, Cp);
    if ((long long)R * g.chunks > 0x7FFFFFFFLL || (long long)R * G > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: R = %d needs more than 2^31 workgroups", who, R);
    return 0;
}

// forward: chunk means and M2 (2, R * chunks, G), then mean and rstd (2, R, G); backward: partial rows (2, R * chunks, Cp), then the two
// group means (2, R, G)
size_t fwd_ws_bytes_of(int R, int G, int chunks) { return ((size_t)2 * R * chunks * G + (size_t)2 * R * G) * sizeof(float); }
size_t bwd_ws_bytes_of(int R, int Cp, int G, int chunks) { return ((size_t)2 * R * chunks * Cp + (size_t)2 * R * G) * sizeof(float); }

}  // namespace

extern "C" int mrcnn_group_norm_map_plan(int R, int H, int W, int C, int Cp, int G, int *pixels_per_chunk, int *chunks, size_t *fwd_ws_bytes,
                                         size_t *bwd_ws_bytes) {
    if (int e = check_geometry("group_norm_map_plan", R, H, W, C, Cp, G)) return e;
    const MapGeom g = map_geom((long long)H * W, Cp);
    if (pixels_per_chunk) *pixels_per_chunk = g.ppc;
    if (chunks) *chunks = g.chunks;
    if (fwd_ws_bytes) *fwd_ws_bytes = fwd_ws_bytes_of(R, G, g.chunks);
    if (bwd_ws_bytes) *bwd_ws_bytes = bwd_ws_bytes_of(R, Cp, G, g.chunks);
    return 0;
}

extern "C" int mrcnn_group_norm_map_fwd_f32(const float *x, const float *gamma, const float *beta, int R, int H, int W, int C, int Cp, int G,
                                            float eps, float *y, float *mean, float *rstd, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "group_norm_map_fwd";
    if (int e = check_geometry(who, R, H, W, C, Cp, G)) return e;
    if (!(eps > 0.f)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: eps must be positive", who);
    if (R == 0) return 0;
    if (!x) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null x", who);
    if (!gamma) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gamma", who);
    if (!beta) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null beta", who);
    if (!y) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null y", who);
    if (!ws) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null workspace", who);
    const int HW = H * W, cpg = C / G;
    const MapGeom g = map_geom(HW, Cp);
    if (ws_bytes < fwd_ws_bytes_of(R, G, g.chunks))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, fwd_ws_bytes_of(R, G, g.chunks));
    if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(y) || !aligned16(ws))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: x, gamma, beta, y and the workspace must be 16-byte aligned", who);
    const float n = (float)((long long)HW * cpg);
    hipStream_t st = (hipStream_t)stream;
    const size_t rkg = (size_t)R * g.chunks * G, rg = (size_t)R * G;
    float *ws_mean = static_cast<float *>(ws), *ws_m2 = ws_mean + rkg, *st_mean = ws_m2 + rkg, *st_rstd = st_mean + rg;
    const dim3 grid((unsigned)(R * g.chunks));
    hipLaunchKernelGGL(k_gnm_stats, grid, dim3(NT), 0, st, x, ws_mean, ws_m2, HW, C, Cp, G, cpg, g.cols, g.rows, g.ppc, g.chunks);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gnm_merge, dim3(mrcnn::cdiv((long long)rg, NT)), dim3(NT), 0, st, ws_mean, ws_m2, st_mean, st_rstd, mean, rstd, R, HW, G,
                       cpg, g.ppc, g.chunks, eps, n);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gnm_apply, grid, dim3(NT), 0, st, x, gamma, beta, st_mean, st_rstd, y, HW, C, Cp, G, cpg, g.cols, g.rows, g.ppc, g.chunks);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_group_norm_map_bwd_f32(const float *gy, const float *x, const float *gamma, const float *mean, const float *rstd, int R, int H,
                                            int W, int C, int Cp, int G, float *gx, float *ggamma, float *gbeta, int accumulate_params, void *ws,
                                            size_t ws_bytes, void *stream) {
    const char *who = "group_norm_map_bwd";
    if (int e = check_geometry(who, R, H, W, C, Cp, G)) return e;
    if (R == 0) return 0;                                     // (no sample: the parameter gradients are left as they are)
    if (!gy) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gy", who);
    if (!x) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null x", who);
    if (!gamma) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gamma", who);
    if (!mean) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null mean", who);
    if (!rstd) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null rstd", who);
    if (!gx) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gx", who);
    if (!ggamma) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null ggamma", who);
    if (!gbeta) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gbeta", who);
    if (!ws) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null workspace", who);
    const int HW = H * W, cpg = C / G;
    const MapGeom g = map_geom(HW, Cp);
    if (ws_bytes < bwd_ws_bytes_of(R, Cp, G, g.chunks))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, bwd_ws_bytes_of(R, Cp, G, g.chunks));
    if (!aligned16(gy) || !aligned16(x) || !aligned16(gamma) || !aligned16(gx) || !aligned16(ggamma) || !aligned16(gbeta) || !aligned16(ws))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: gy, x, gamma, gx, ggamma, gbeta and the workspace must be 16-byte aligned", who);
    const float n = (float)((long long)HW * cpg);
    hipStream_t st = (hipStream_t)stream;
    const size_t rkc = (size_t)R * g.chunks * Cp, rg = (size_t)R * G;
    float *ws1 = static_cast<float *>(ws), *ws2 = ws1 + rkc, *ws_a = ws2 + rkc, *ws_b = ws_a + rg;
    const dim3 grid((unsigned)(R * g.chunks));
    hipLaunchKernelGGL(k_gnm_bwd_sums, grid, dim3(NT), 0, st, gy, x, mean, rstd, ws1, ws2, HW, C, Cp, G, cpg, g.cols, g.rows, g.ppc, g.chunks);
    MRCNN_LAUNCH_CHECK();
    const int gpb = NT / cpg;
    hipLaunchKernelGGL(k_gnm_bwd_final, dim3(mrcnn::cdiv(G, gpb)), dim3(NT), 0, st, ws1, ws2, gamma, ws_a, ws_b, ggamma, gbeta, R, C, Cp, G, cpg, gpb,
                       g.chunks, accumulate_params, n);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gnm_bwd_dx, grid, dim3(NT), 0, st, gy, x, gamma, mean, rstd, ws_a, ws_b, gx, HW, C, Cp, G, cpg, g.cols, g.rows, g.ppc,
                       g.chunks);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
