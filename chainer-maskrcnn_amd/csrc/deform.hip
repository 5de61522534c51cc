// Deformable convolution (Dai et al. 2017; modulated: Zhu et al. 2019) on the device for gfx950: the sampling around the 3x3 layers of
// res3-res5, whose GEMMs stay the library's.  No counterpart in the reference.
//   mrcnn_deform_cols_fwd_f32     x + offsets -> cols (N,H,W,9*C), tap-major: the operand of a 1x1 convolution over 9*C channels
//   mrcnn_deform_offset_bwd_f32   g_cols, x, offsets -> the gradient of the whole padded offset row (pads written as zeros)
//   mrcnn_deform_input_bwd_f32    g_cols, offsets -> the gradient of x, without float atomics: an inverted index per call (count with
//                                 integer atomics, exclusive scan, fill), then one wave per destination pixel that orders its list and sums
//                                 it in ascending (source pixel, tap, corner) order; the same bits on every run
// Every position, corner and weight follows the one rule of deform_common.h.  float32 without contraction.  Restated in torch float64 by
// tests/deform_reference.py.
#include "common.h"
#include "deform_common.h"
#include <algorithm>
#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int DT = 256;                  // threads of the streaming kernels: four waves, one (pixel, tap) each
constexpr int DW = DT / 64;
constexpr int LIST_MAX = 256;            // entries the one-wave kernel orders in LDS (the mean list is 36 long)
constexpr int LONG_T = 512;              // threads of the workgroup that takes a longer list
constexpr int LONG_WAVES = LONG_T / 64;
constexpr int LONG_CHUNK = 128;          // a long list is summed in chunks of this many entries, the partial sums added in chunk order
constexpr int LONG_GRID = 32;            // workgroups that share the long lists (each takes every LONG_GRID-th of them)
constexpr int SCAN_T = 1024;
constexpr int C_MAX = 512;               // two float4 accumulators per lane
static_assert(C_MAX <= LONG_T && C_MAX <= 2 * 64 * 4, "a thread per channel in the long-list kernel, two float4s per lane");

struct TapGeom { DeformCorners t; float m; };

// tap k of source pixel s = (n, y, x): its corners and its modulation
__device__ __forceinline__ TapGeom tap_geom(const float *__restrict__ off, int ld, int modulated, long long s, int k, int H, int W) {
    const int x = (int)(s % W), y = (int)((s / W) % H);
    const float *o = off + (size_t)s * ld;
    TapGeom g;
    g.t = deform_corners(deform_pos_y(y, k, o[2 * k]), deform_pos_x(x, k, o[2 * k + 1]), H, W);
    g.m = modulated ? sigmoid1(o[kDeformOffsetCh + k]) : 1.0f;
    return g;
}

__device__ __forceinline__ size_t cell(const DeformCorners &t, int c, int W) { return (size_t)(t.y0 + (c >> 1)) * W + (t.x0 + (c & 1)); }

__device__ __forceinline__ float4 corner4(const DeformCorners &t, int c, const float *__restrict__ img, int W, int C, int q) {
    return (t.valid >> c) & 1u ? ld4(img + cell(t, c, W) * C + 4 * q) : f4(0.f);
}

// ---- columns ------------------------------------------------------------------------------------------------------------------------------
// GL lanes per (pixel, tap) - a wave, or half of one where C / 4 <= 32 would leave the other half idle; the corners and weights are uniform
// over those lanes, which run over the float4s of the C channels.
template <int GL>
__global__ __launch_bounds__(DT) void k_deform_cols(const float *__restrict__ x, const float *__restrict__ off, int ld, int modulated, int H,
                                                    int W, int C, long long n_items, float *__restrict__ cols) {
    constexpr int IW = 64 / GL;
    const int gl = (threadIdx.x & 63) % GL, C4 = C >> 2;
    for (long long it = ((long long)blockIdx.x * DW + (threadIdx.x >> 6)) * IW + (threadIdx.x & 63) / GL; it < n_items;
         it += (long long)gridDim.x * DW * IW) {
        const long long s = it / kDeformTaps;
        const int k = (int)(it % kDeformTaps);
        const TapGeom g = tap_geom(off, ld, modulated, s, k, H, W);
        const float *img = x + (size_t)(s / ((long long)H * W)) * H * W * C;
        const float w0 = deform_weight(g.t, 0), w1 = deform_weight(g.t, 1), w2 = deform_weight(g.t, 2), w3 = deform_weight(g.t, 3);
        float *o = cols + (size_t)it * C;
        for (int q = gl; q < C4; q += GL) {
            float4 v = f4(0.f);
            if (g.t.valid) {
                const float4 a = corner4(g.t, 0, img, W, C, q), b = corner4(g.t, 1, img, W, C, q), c = corner4(g.t, 2, img, W, C, q),
                             d = corner4(g.t, 3, img, W, C, q);
                v.x = (((w0 * a.x + w1 * b.x) + w2 * c.x) + w3 * d.x) * g.m;
                v.y = (((w0 * a.y + w1 * b.y) + w2 * c.y) + w3 * d.y) * g.m;
                v.z = (((w0 * a.z + w1 * b.z) + w2 * c.z) + w3 * d.z) * g.m;
                v.w = (((w0 * a.w + w1 * b.w) + w2 * c.w) + w3 * d.w) * g.m;
            }
            st4(o + 4 * q, v);
        }
    }
}

// ---- offset and mask gradient ---------------------------------------------------------------------------------------------------------------
template <int GL>
__device__ __forceinline__ float group_sum(float v) {      // a butterfly over GL aligned lanes: the same order on every run
#pragma unroll
    for (int d = GL / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// GL lanes per (pixel, tap), as above: three sums over the channels, reduced over those lanes; the lanes of tap 0 also write the zeros of
// the padded channels, so every channel of the row is written exactly once.
template <int GL>
__global__ __launch_bounds__(DT) void k_deform_offset_bwd(const float *__restrict__ g_cols, const float *__restrict__ x,
                                                          const float *__restrict__ off, int ld, int modulated, int H, int W, int C,
                                                          long long n_items, float *__restrict__ g_off) {
    constexpr int IW = 64 / GL;
    const int gl = (threadIdx.x & 63) % GL, C4 = C >> 2;
    const int used = modulated ? kDeformOffsetCh + kDeformTaps : kDeformOffsetCh;
    for (long long it = ((long long)blockIdx.x * DW + (threadIdx.x >> 6)) * IW + (threadIdx.x & 63) / GL; it < n_items;
         it += (long long)gridDim.x * DW * IW) {
        const long long s = it / kDeformTaps;
        const int k = (int)(it % kDeformTaps);
        const TapGeom g = tap_geom(off, ld, modulated, s, k, H, W);
        float ady = 0.f, adx = 0.f, as = 0.f;
        if (g.t.valid) {
            const float *img = x + (size_t)(s / ((long long)H * W)) * H * W * C;
            const float *gc = g_cols + (size_t)it * C;
            const float w0 = deform_weight(g.t, 0), w1 = deform_weight(g.t, 1), w2 = deform_weight(g.t, 2), w3 = deform_weight(g.t, 3);
            for (int q = gl; q < C4; q += GL) {
                const float4 a = corner4(g.t, 0, img, W, C, q), b = corner4(g.t, 1, img, W, C, q), c = corner4(g.t, 2, img, W, C, q),
                             d = corner4(g.t, 3, img, W, C, q), gv = ld4(gc + 4 * q);
#define DEFORM_TERM(f)                                                                                     \
                ady += gv.f * (g.t.hx * (c.f - a.f) + g.t.lx * (d.f - b.f));                                 \
                adx += gv.f * (g.t.hy * (b.f - a.f) + g.t.ly * (d.f - c.f));                                 \
                as += gv.f * (((w0 * a.f + w1 * b.f) + w2 * c.f) + w3 * d.f);
                DEFORM_TERM(x) DEFORM_TERM(y) DEFORM_TERM(z) DEFORM_TERM(w)
#undef DEFORM_TERM
            }
        }
        ady = group_sum<GL>(ady);
        adx = group_sum<GL>(adx);
        as = group_sum<GL>(as);
        float *o = g_off + (size_t)s * ld;
        if (gl == 0) {
            o[2 * k] = g.m * ady;
            o[2 * k + 1] = g.m * adx;
            if (modulated) o[kDeformOffsetCh + k] = (g.m * (1.0f - g.m)) * as;
        }
        if (k == 0)
            for (int c = used + gl; c < ld; c += GL) o[c] = 0.f;
    }
}

// ---- input gradient: the inverted index ---------------------------------------------------------------------------------------------------
// A thread per (source pixel, tap).  FILL = false counts the entries of every destination (integer atomics: a count does not depend on the
// order of arrival); FILL = true writes the entry ids into the destinations' lists, in whatever order the atomics hand the slots out.
template <bool FILL>
__global__ __launch_bounds__(DT) void k_deform_index(const float *__restrict__ off, int ld, int modulated, int H, int W, long long n_items,
                                                     int *__restrict__ count, const int *__restrict__ start, int *__restrict__ list) {
    for (long long it = (long long)blockIdx.x * DT + threadIdx.x; it < n_items; it += (long long)gridDim.x * DT) {
        const long long s = it / kDeformTaps;
        const int k = (int)(it % kDeformTaps);
        const DeformCorners t = tap_geom(off, ld, 0, s, k, H, W).t;
        if (!t.valid) continue;
        const long long img0 = s / ((long long)H * W) * H * W;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if ((t.valid >> c) & 1u) {
                const long long d = img0 + (long long)cell(t, c, W);
                const int slot = atomicAdd(count + d, 1);
                if (FILL) list[start[d] + slot] = (int)(it * 4 + c);
            }
    }
}

// One workgroup: start = the exclusive scan of count (start[P] = the total), and the destinations whose list is longer than LIST_MAX.
__global__ __launch_bounds__(SCAN_T) void k_deform_scan(const int *__restrict__ count, int P, int *__restrict__ start, int *__restrict__ n_long,
                                                        int *__restrict__ long_ids) {
    __shared__ int s1[SCAN_T], s2[SCAN_T];
    const int t = threadIdx.x;
    const int per = (P + SCAN_T - 1) / SCAN_T;
    const int i0 = min(P, t * per), i1 = min(P, i0 + per);
    int a = 0, b = 0;
    for (int i = i0; i < i1; ++i) { a += count[i]; b += count[i] > LIST_MAX ? 1 : 0; }
    s1[t] = a; s2[t] = b;
    __syncthreads();
    for (int d = 1; d < SCAN_T; d <<= 1) {
        const int u = t >= d ? s1[t - d] : 0, v = t >= d ? s2[t - d] : 0;
        __syncthreads();
        s1[t] += u; s2[t] += v;
        __syncthreads();
    }
    int ra = s1[t] - a, rb = s2[t] - b;
    for (int i = i0; i < i1; ++i) {
        const int c = count[i];
        start[i] = ra;
        ra += c;
        if (c > LIST_MAX) long_ids[rb++] = i;
    }
    if (t == 0) { start[P] = s1[SCAN_T - 1]; *n_long = s2[SCAN_T - 1]; }
}

// Ascending order of n entries by T threads (tid = this thread): a bitonic network whose comparators all point the same way, so the
// entries past n may be thought of as +infinity and their comparators skipped; n need not be a power of two.
template <int T>
__device__ __forceinline__ void sort_entries(int *e, int n, int tid) {
    for (int k = 2; (k >> 1) < n; k <<= 1) {
        for (int i = tid; i < n; i += T) {
            const int o = i ^ (k - 1);
            if (o > i && o < n) { const int a = e[i], b = e[o]; if (a > b) { e[i] = b; e[o] = a; } }
        }
        __syncthreads();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int i = tid; i < n; i += T) {
                const int o = i ^ j;
                if (o > i && o < n) { const int a = e[i], b = e[o]; if (a > b) { e[i] = b; e[o] = a; } }
            }
            __syncthreads();
        }
    }
}

// orders one wave's own LDS writes before its reads of them (the waves of the long-list workgroup do not arrive together)
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a += w * g with the rounding error of the addition carried in c (Kahan; no contraction, no reassociation in this build): a plain
// float32 sequence over a few hundred entries loses 5e-7 - 7e-7 of max|gx|, more than four times what a float32 reference loses.
__device__ __forceinline__ void add1(float &a, float &c, float v) {
    const float y = v - c, t = a + y;
    c = (t - a) - y;
    a = t;
}
__device__ __forceinline__ void add_entry(float4 &a, float4 &c, float w, const float4 g) {
    add1(a.x, c.x, w * g.x); add1(a.y, c.y, w * g.y); add1(a.z, c.z, w * g.z); add1(a.w, c.w, w * g.w);
}

// Entries e[0 .. n) of one wave (ascending) added into (a0, a1), the float4s lane and lane + 64 of the C channels: the lanes first work out
// the weight and the g_cols row of 64 entries, one each, then all of them walk those 64 in order.  wv / rw: 64 floats / ints of LDS per wave.
__device__ __forceinline__ void sum_entries(const int *e, int n, const float *__restrict__ g_cols, const float *__restrict__ off, int ld,
                                            int modulated, int H, int W, int C, int lane, float *wv, int *rw, float4 &a0, float4 &a1) {
    const int C4 = C >> 2;
    const bool two = lane + 64 < C4, one = lane < C4;
    float4 c0 = f4(0.f), c1 = f4(0.f);       // what the float32 additions so far have lost (compensated summation, still in entry order)
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        if (i < n) {
            const int id = e[i], c = id & 3, sk = id >> 2;
            const TapGeom g = tap_geom(off, ld, modulated, sk / kDeformTaps, sk % kDeformTaps, H, W);
            wv[lane] = deform_weight(g.t, c) * g.m;
            rw[lane] = sk;
        }
        wave_fence();
        const int cnt = min(64, n - base);
        if (one) {
            // four rows in flight at a time; the additions stay in entry order
            int j = 0;
            for (; j + 4 <= cnt; j += 4) {
                float4 g[4], h[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float *r = g_cols + (size_t)rw[j + u] * C;
                    g[u] = ld4(r + 4 * lane);
                    h[u] = two ? ld4(r + 4 * (lane + 64)) : f4(0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    add_entry(a0, c0, wv[j + u], g[u]);
                    if (two) add_entry(a1, c1, wv[j + u], h[u]);
                }
            }
            for (; j < cnt; ++j) {
                const float *r = g_cols + (size_t)rw[j] * C;
                add_entry(a0, c0, wv[j], ld4(r + 4 * lane));
                if (two) add_entry(a1, c1, wv[j], ld4(r + 4 * (lane + 64)));
            }
        }
        wave_fence();
    }
}

__device__ __forceinline__ float4 relu_mask4(float4 v, float4 x) {
    return make_float4(x.x > 0.f ? v.x : 0.f, x.y > 0.f ? v.y : 0.f, x.z > 0.f ? v.z : 0.f, x.w > 0.f ? v.w : 0.f);
}

// A wave (a workgroup of one) per destination pixel with a list of at most LIST_MAX entries: the list is ordered in LDS, the prior value
// of gx (accumulate) is the first addend, the ReLU mask of the layer's input is applied to the total.
__global__ __launch_bounds__(64) void k_deform_gather(const float *__restrict__ g_cols, const float *__restrict__ off, int ld, int modulated,
                                                      int H, int W, int C, int P, const int *__restrict__ start,
                                                      const int *__restrict__ list, float *__restrict__ gx, const float *__restrict__ relu_x,
                                                      int accumulate) {
    __shared__ int ent[LIST_MAX];
    __shared__ float wv[64];
    __shared__ int rw[64];
    const int lane = threadIdx.x, C4 = C >> 2;
    for (int d = blockIdx.x; d < P; d += gridDim.x) {
        const int b = start[d], n = start[d + 1] - b;
        if (n > LIST_MAX) continue;             // k_deform_gather_long's
        if (n <= 64) {                          // the usual list: every lane counts the entries below its own
            const int mine = lane < n ? list[b + lane] : INT_MAX;
            ent[lane] = mine;
            __syncthreads();
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += ent[j] < mine ? 1 : 0;
            __syncthreads();
            if (lane < n) ent[rank] = mine;
            __syncthreads();
        } else {
            for (int i = lane; i < n; i += 64) ent[i] = list[b + i];
            __syncthreads();
            sort_entries<64>(ent, n, lane);
        }
        float *o = gx + (size_t)d * C;
        float4 a0 = f4(0.f), a1 = f4(0.f);
        if (accumulate) {
            if (lane < C4) a0 = ld4(o + 4 * lane);
            if (lane + 64 < C4) a1 = ld4(o + 4 * (lane + 64));
        }
        sum_entries(ent, n, g_cols, off, ld, modulated, H, W, C, lane, wv, rw, a0, a1);
        if (lane < C4) st4(o + 4 * lane, relu_x ? relu_mask4(a0, ld4(relu_x + (size_t)d * C + 4 * lane)) : a0);
        if (lane + 64 < C4) st4(o + 4 * (lane + 64), relu_x ? relu_mask4(a1, ld4(relu_x + (size_t)d * C + 4 * (lane + 64))) : a1);
        __syncthreads();                        // the next destination reuses ent
    }
}

// A workgroup per destination with a longer list: the list is ordered in place in global memory; the waves then take chunks of LONG_CHUNK
// entries, LONG_WAVES at a time, and the partial sums are added to the total in chunk order.
__global__ __launch_bounds__(LONG_T) void k_deform_gather_long(const float *__restrict__ g_cols, const float *__restrict__ off, int ld,
                                                               int modulated, int H, int W, int C, const int *__restrict__ start,
                                                               int *__restrict__ list, const int *__restrict__ n_long,
                                                               const int *__restrict__ long_ids, float *__restrict__ gx,
                                                               const float *__restrict__ relu_x, int accumulate) {
    __shared__ float part[LONG_WAVES * C_MAX];
    __shared__ float wv[LONG_WAVES * 64];
    __shared__ int rw[LONG_WAVES * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, C4 = C >> 2;
    const int nl = *n_long;
    for (int li = blockIdx.x; li < nl; li += gridDim.x) {       // (uniform over the workgroup)
    const int d = long_ids[li];
    const int b = start[d], n = start[d + 1] - b;
    int *e = list + b;
    sort_entries<LONG_T>(e, n, tid);
    float total = (accumulate && tid < C) ? gx[(size_t)d * C + tid] : 0.f;      // thread c keeps channel c
    const int n_chunks = (n + LONG_CHUNK - 1) / LONG_CHUNK;
    for (int c0 = 0; c0 < n_chunks; c0 += LONG_WAVES) {
        const int ch = c0 + wave;
        if (ch < n_chunks) {
            float4 a0 = f4(0.f), a1 = f4(0.f);
            sum_entries(e + ch * LONG_CHUNK, min(LONG_CHUNK, n - ch * LONG_CHUNK), g_cols, off, ld, modulated, H, W, C, lane, wv + wave * 64,
                        rw + wave * 64, a0, a1);
            float *p = part + wave * C_MAX;
            if (lane < C4) *reinterpret_cast<float4 *>(p + 4 * lane) = a0;
            if (lane + 64 < C4) *reinterpret_cast<float4 *>(p + 4 * (lane + 64)) = a1;
        }
        __syncthreads();
        if (tid < C)
            for (int w = 0; w < LONG_WAVES && c0 + w < n_chunks; ++w) total += part[w * C_MAX + tid];
        __syncthreads();
    }
    if (tid < C) gx[(size_t)d * C + tid] = (relu_x && !(relu_x[(size_t)d * C + tid] > 0.f)) ? 0.f : total;
    }
}

int blocks_for(long long work, int per_block) {
    return (int)std::max<long long>(1, std::min<long long>((work + per_block - 1) / per_block, 1 << 20));
}

// what every entry point refuses: the geometry first (UNSUPPORTED), then sizes
int check_geometry(const char *who, int N, int H, int W, int C, int ld_off, int modulated, int KH, int KW, int stride, int pad, int dilation,
                   int groups) {
    if (KH != 3 || KW != 3 || stride != 1 || pad != 1 || dilation != 1 || groups != 1)
        return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "%s: a %d x %d layer of stride %d, pad %d, dilation %d, %d deformable groups (3 x 3, 1, 1, 1, 1 only)",
                               who, KH, KW, stride, pad, dilation, groups);
    if (modulated != 0 && modulated != 1) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: modulated must be 0 or 1, got %d", who, modulated);
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || (C % 4)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad sizes (N >= 0; H, W, C > 0; C a multiple of 4)", who);
    const int used = kDeformOffsetCh + (modulated ? kDeformTaps : 0);
    if (ld_off < used) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: an offset row stride (ld_off) of %d, %d channels are read", who, ld_off, used);
    if (H > (1 << 20) || W > (1 << 20) || (long long)N * H * W * 36 > INT_MAX)
        return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "%s: map too large (N * H * W * 36 must fit int32)", who);
    return 0;
}

bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

struct IndexLayout { size_t count, cursor, start, n_long, long_ids, list, ints; };
IndexLayout index_layout(long long P) {
    auto up = [](size_t v) { return (v + 3) / 4 * 4; };
    IndexLayout l;
    l.count = 0;
    l.cursor = up((size_t)P);
    l.start = l.cursor + up((size_t)P);
    l.n_long = l.start + up((size_t)P + 1);
    l.long_ids = l.n_long + 4;
    l.list = l.long_ids + up((size_t)(36 * P / (LIST_MAX + 1) + 1));
    l.ints = l.list + up((size_t)36 * P);
    return l;
}

}  // namespace

extern "C" int mrcnn_deform_cols_fwd_f32(const float *x, const float *off, int ld_off, int modulated, int N, int H, int W, int C, int KH, int KW,
                                         int stride, int pad, int dilation, int groups, float *cols, void *stream) {
    if (int rc = check_geometry("deform_cols_fwd", N, H, W, C, ld_off, modulated, KH, KW, stride, pad, dilation, groups)) return rc;
    if (N == 0) return 0;
    if (!x || !off || !cols) return mrcnn::fail_arg(MRCNN_E_INVALID, "deform_cols_fwd: null pointer (x, off, cols)");
    if (misaligned(x) || misaligned(cols)) return mrcnn::fail_arg(MRCNN_E_INVALID, "deform_cols_fwd: x and cols must be 16-byte aligned");
    const long long n_items = (long long)N * H * W * kDeformTaps;
    if (C / 4 <= 32)
        hipLaunchKernelGGL(k_deform_cols<32>, dim3(blocks_for(n_items, 2 * DW)), dim3(DT), 0, (hipStream_t)stream, x, off, ld_off, modulated, H, W, C,
                           n_items, cols);
    else
        hipLaunchKernelGGL(k_deform_cols<64>, dim3(blocks_for(n_items, DW)), dim3(DT), 0, (hipStream_t)stream, x, off, ld_off, modulated, H, W, C,
                           n_items, cols);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_deform_offset_bwd_f32(const float *g_cols, const float *x, const float *off, int ld_off, int modulated, int N, int H, int W,
                                           int C, int KH, int KW, int stride, int pad, int dilation, int groups, float *g_off, void *stream) {
    if (int rc = check_geometry("deform_offset_bwd", N, H, W, C, ld_off, modulated, KH, KW, stride, pad, dilation, groups)) return rc;
    if (N == 0) return 0;
    if (!g_cols || !x || !off || !g_off) return mrcnn::fail_arg(MRCNN_E_INVALID, "deform_offset_bwd: null pointer (g_cols, x, off, g_off)");
    if (misaligned(x) || misaligned(g_cols)) return mrcnn::fail_arg(MRCNN_E_INVALID, "deform_offset_bwd: x and g_cols must be 16-byte aligned");
    const long long n_items = (long long)N * H * W * kDeformTaps;
    if (C / 4 <= 32)
        hipLaunchKernelGGL(k_deform_offset_bwd<32>, dim3(blocks_for(n_items, 2 * DW)), dim3(DT), 0, (hipStream_t)stream, g_cols, x, off, ld_off,
                           modulated, H, W, C, n_items, g_off);
    else
        hipLaunchKernelGGL(k_deform_offset_bwd<64>, dim3(blocks_for(n_items, DW)), dim3(DT), 0, (hipStream_t)stream, g_cols, x, off, ld_off,
                           modulated, H, W, C, n_items, g_off);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mrcnn_deform_input_bwd_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || (long long)N * H * W * 36 > INT_MAX) return 0;
    return index_layout((long long)N * H * W).ints * sizeof(int);
}

extern "C" int mrcnn_deform_input_bwd_f32(const float *g_cols, const float *off, int ld_off, int modulated, int N, int H, int W, int C, int KH,
                                          int KW, int stride, int pad, int dilation, int groups, float *gx, const float *relu_x, int accumulate,
                                          void *ws, size_t ws_bytes, void *stream) {
    if (int rc = check_geometry("deform_input_bwd", N, H, W, C, ld_off, modulated, KH, KW, stride, pad, dilation, groups)) return rc;
    if (C > C_MAX) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "deform_input_bwd: %d channels (at most %d)", C, C_MAX);
    if (accumulate != 0 && accumulate != 1) return mrcnn::fail_arg(MRCNN_E_INVALID, "deform_input_bwd: accumulate must be 0 or 1, got %d", accumulate);
    if (N == 0) return 0;
    if (!g_cols || !off || !gx) return mrcnn::fail_arg(MRCNN_E_INVALID, "deform_input_bwd: null pointer (g_cols, off, gx)");
    if (misaligned(g_cols) || misaligned(gx) || misaligned(relu_x) || misaligned(ws))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "deform_input_bwd: g_cols, gx, relu_x and ws must be 16-byte aligned");
    const long long P = (long long)N * H * W;
    const IndexLayout l = index_layout(P);
    if (!ws || ws_bytes < l.ints * sizeof(int)) return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "deform_input_bwd: workspace too small (%zu bytes needed)", l.ints * sizeof(int));
    hipStream_t st = (hipStream_t)stream;
    int *w = (int *)ws;
    int *count = w + l.count, *cursor = w + l.cursor, *start = w + l.start, *n_long = w + l.n_long, *long_ids = w + l.long_ids, *list = w + l.list;
    MRCNN_HIP_TRY(hipMemsetAsync(w, 0, l.start * sizeof(int), st));        // count and cursor
    const long long n_items = P * kDeformTaps;
    hipLaunchKernelGGL(k_deform_index<false>, dim3(blocks_for(n_items, DT)), dim3(DT), 0, st, off, ld_off, modulated, H, W, n_items, count,
                       (const int *)nullptr, (int *)nullptr);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_deform_scan, dim3(1), dim3(SCAN_T), 0, st, (const int *)count, (int)P, start, n_long, long_ids);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_deform_index<true>, dim3(blocks_for(n_items, DT)), dim3(DT), 0, st, off, ld_off, modulated, H, W, n_items, cursor,
                       (const int *)start, list);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_deform_gather, dim3(blocks_for(P, 1)), dim3(64), 0, st, g_cols, off, ld_off, modulated, H, W, C, (int)P,
                       (const int *)start, (const int *)list, gx, relu_x, accumulate);
    MRCNN_LAUNCH_CHECK();
    const int max_long = (int)(36 * P / (LIST_MAX + 1));        // no more destinations can hold more than LIST_MAX entries each
    if (max_long > 0) {
        hipLaunchKernelGGL(k_deform_gather_long, dim3(std::min(max_long, LONG_GRID)), dim3(LONG_T), 0, st, g_cols, off, ld_off, modulated, H, W, C, (const int *)start,
                           list, (const int *)n_long, (const int *)long_ids, gx, relu_x, accumulate);
        MRCNN_LAUNCH_CHECK();
    }
    return 0;
}
