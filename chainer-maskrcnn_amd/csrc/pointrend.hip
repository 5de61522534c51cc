// PointRend (Kirillov et al., CVPR 2020) on the device for gfx950: the per-point work around the point head, whose four 1x1 layers run as
// the library's GEMMs.  No counterpart in the reference, whose mask is the 28 x 28 grid.
//   mrcnn_point_train_coords   keys + coarse logits -> the training points of every mask row: candidates, uncertainty, a ranked selection
//                              in LDS, the uniform remainder; one launch, one workgroup per row
//   mrcnn_point_features_fwd   points -> the head's input: the stride-4 map and the row's coarse logits sampled at every point
//   mrcnn_point_features_bwd   the fine part of the input gradient added into the map's gradient, owner-computes, the same bits every run
//   mrcnn_point_concat_fwd     a hidden layer's output + the coarse channels of the head's input -> the next layer's input
//   mrcnn_point_concat_bwd     the hidden part of that input's gradient (the coarse part is dropped: the coarse logits are a constant)
//   mrcnn_point_target         the ground-truth mask sampled at the points; -1 marks a row that is not live
//   mrcnn_point_bce            sigmoid cross entropy over the live rows' points as a (sum, count) row of loss.hip's form
//   mrcnn_point_subdivide      2x upsample of a logit grid, the most uncertain cells and their centres; one workgroup per detection
//   mrcnn_point_scatter        the head's predictions written into those cells
// Every sample follows the one rule of point_common.h.  float32 without contraction, no float atomics.  Restated in NumPy by
// tests/pointrend_reference.py.
#include "point_common.h"
#include "loss_common.h"

#pragma clang fp contract(off)

namespace {

struct Roi5 { float idx, x1, y1, x2, y2; };
__device__ __forceinline__ Roi5 load_roi(const float *__restrict__ rois, int r) {
    const float *p = rois + (size_t)r * 5;
    return Roi5{p[0], p[1], p[2], p[3], p[4]};
}
// frame position of the normalised point (u, v) of a box
__device__ __forceinline__ void point_frame(const Roi5 &b, float u, float v, float &X, float &Y) {
    X = b.x1 + u * (b.x2 - b.x1);
    Y = b.y1 + v * (b.y2 - b.y1);
}

// ---- training points ------------------------------------------------------------------------------------------------------------------
constexpr int PT_MAX_CAND = 4096;       // candidates per row the LDS sort holds (the default is 3 * 196 = 588)

// One workgroup per row.  Candidate j takes the keys 2j (u) and 2j + 1 (v) of the row; its sort key is (bits of |coarse logit at it|, j),
// ascending - the most uncertain first, ties to the lower index.  A row whose label selects no channel has uncertainty 0 everywhere, so its
// first n_imp candidates are taken in index order.  Points n_imp .. P-1 take the keys behind the candidates'.
__global__ __launch_bounds__(NT) void k_point_train_coords(const uint32_t *__restrict__ keys, int n_keys, const float *__restrict__ coarse,
                                                           int S0, int Cp, int n_channels, const int32_t *__restrict__ label, int label_base,
                                                           int P, int n_cand, int n_imp, int n2, float *__restrict__ coords) {
    __shared__ unsigned long long sk[PT_MAX_CAND];
    const int r = blockIdx.x;
    const uint32_t *kr = keys + (size_t)r * n_keys;
    const int ch = label[r] - label_base;
    const bool has = ch >= 0 && ch < n_channels;
    const float *lg = coarse + (size_t)r * S0 * S0 * Cp + (has ? ch : 0);
    for (int j = threadIdx.x; j < n2; j += NT) {
        unsigned long long k = ~0ull;
        if (j < n_cand) {
            float val = 0.f;
            if (has) {
                const PointTaps t = point_taps(point_unit(kr[2 * j]) * (float)S0, point_unit(kr[2 * j + 1]) * (float)S0, S0, S0);
                val = point_sample(t, S0, S0, [&](int y, int x) { return lg[((size_t)y * S0 + x) * Cp]; });
            }
            k = ((unsigned long long)__float_as_uint(fabsf(val)) << 32) | (unsigned)j;
        }
        sk[j] = k;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += NT) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long a = sk[i], b = sk[o];
                    if ((a > b) == ((i & k) == 0)) { sk[i] = b; sk[o] = a; }
                }
            }
            __syncthreads();
        }
    float *out = coords + (size_t)r * P * 2;
    for (int p = threadIdx.x; p < P; p += NT) {
        const int k0 = p < n_imp ? 2 * (int)(sk[p] & 0xffffffffu) : 2 * n_cand + 2 * (p - n_imp);
        out[2 * p] = point_unit(kr[k0]);
        out[2 * p + 1] = point_unit(kr[k0 + 1]);
    }
}

// ---- the head's input -----------------------------------------------------------------------------------------------------------------
// A wave per point, lanes over the float4s of the output row: [0, C) the map at (X * scale, Y * scale) - one contiguous run of C floats per
// tap -, [C, C + n_channels) the row's coarse logits at (u * S0, v * S0), zeros behind them.
__global__ __launch_bounds__(NT) void k_point_features_fwd(const float *__restrict__ coords, const float *__restrict__ rois,
                                                           const float *__restrict__ map, int N, int H, int W, int C, float scale,
                                                           const float *__restrict__ coarse, int S0, int Cp, int n_channels,
                                                           long long n_points, int P, int cin_p, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int C4 = C >> 2, cin4 = cin_p >> 2;
    for (long long pt = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); pt < n_points; pt += (long long)gridDim.x * (NT / 64)) {
        const int r = (int)(pt / P);
        const Roi5 b = load_roi(rois, r);
        const float u = coords[pt * 2], v = coords[pt * 2 + 1];
        float X, Y;
        point_frame(b, u, v, X, Y);
        const PointTaps tf = point_taps(X * scale, Y * scale, W, H);
        const PointTaps tc = point_taps(u * (float)S0, v * (float)S0, S0, S0);
        const bool img_ok = b.idx >= 0.f && b.idx < (float)N;
        const float *mp = map + (size_t)(img_ok ? (int)b.idx : 0) * H * W * C;
        const float *cp = coarse + (size_t)r * S0 * S0 * Cp;
        float *o = out + (size_t)pt * cin_p;
        for (int q = lane; q < cin4; q += 64) {
            float4 s = f4(0.f);
            if (q < C4) {
                if (img_ok) s = point_sample4(tf, W, H, mp + 4 * q, (size_t)C);
            } else {
                const int c0 = 4 * (q - C4);
                if (c0 < n_channels) {
                    s = point_sample4(tc, S0, S0, cp + c0, (size_t)Cp);
                    if (c0 + 1 >= n_channels) s.y = 0.f;
                    if (c0 + 2 >= n_channels) s.z = 0.f;
                    if (c0 + 3 >= n_channels) s.w = 0.f;
                }
            }
            st4(o + 4 * q, s);
        }
    }
}

// ---- its backward into the map --------------------------------------------------------------------------------------------------------
// Owner-computes: a wave owns a patch of PB_H x PB_W cells of one image's gradient map and keeps their sums in LDS (a float4 per lane and
// cell, so no two lanes share an address).  It scans the rows of its image whose box, in map coordinates and widened by one cell, touches
// the patch - 64 rows per ballot -, then those rows' points - 64 per ballot -, and adds w * g for every tap that lands on its cells, in
// ascending (row, point) order and tap order 00, 01, 10, 11.  The value the map held is the FIRST addend: the patch is loaded when the first
// tap lands on it, and written once at the end; a patch no tap lands on is neither read nor written.
constexpr int PB_H = 2, PB_W = 4, PB_CELLS = PB_H * PB_W, PB_WAVES = NT / 64;

__global__ __launch_bounds__(NT) void k_point_features_bwd(const float *__restrict__ g_in, int ld, const float *__restrict__ coords,
                                                           const float *__restrict__ rois, int rows, int P, float scale,
                                                           float *__restrict__ g_map, int H, int W, int C, int tiles_x, int tiles_y,
                                                           long long n_patches) {
    extern __shared__ float4 pb_acc[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long patch = (long long)blockIdx.x * PB_WAVES + wave;
    if (patch >= n_patches) return;         // (no workgroup barrier in this kernel)
    const int C4 = C >> 2;
    const int img = (int)(patch / ((long long)tiles_x * tiles_y));
    const int rem = (int)(patch % ((long long)tiles_x * tiles_y));
    const int py0 = (rem / tiles_x) * PB_H, px0 = (rem % tiles_x) * PB_W;
    const int ye = min(py0 + PB_H, H), xe = min(px0 + PB_W, W);
    float4 *acc = pb_acc + (size_t)wave * PB_CELLS * C4;
    float *gm = g_map + (size_t)img * H * W * C;
    bool loaded = false;
    for (int r0 = 0; r0 < rows; r0 += 64) {
        const int r = r0 + lane;
        bool ov = false;
        if (r < rows) {
            const Roi5 b = load_roi(rois, r);
            if (b.idx == (float)img) {
                const float lx = floorf(fminf(b.x1, b.x2) * scale) - 1.f, hx = floorf(fmaxf(b.x1, b.x2) * scale) + 1.f;
                const float ly = floorf(fminf(b.y1, b.y2) * scale) - 1.f, hy = floorf(fmaxf(b.y1, b.y2) * scale) + 1.f;
                ov = !(hx < (float)px0 || lx > (float)(xe - 1) || hy < (float)py0 || ly > (float)(ye - 1));
            }
        }
        unsigned long long rmask = __ballot(ov);
        while (rmask) {
            const int rr = r0 + __ffsll((long long)rmask) - 1;
            rmask &= rmask - 1;
            const Roi5 b = load_roi(rois, rr);
            for (int p0 = 0; p0 < P; p0 += 64) {
                const int p = p0 + lane;
                bool hit = false;
                if (p < P) {
                    const float *c = coords + ((size_t)rr * P + p) * 2;
                    float X, Y;
                    point_frame(b, c[0], c[1], X, Y);
                    const PointTaps t = point_taps(X * scale, Y * scale, W, H);
                    hit = t.x0 + 1 >= px0 && t.x0 < xe && t.y0 + 1 >= py0 && t.y0 < ye;
                }
                unsigned long long hmask = __ballot(hit);
                while (hmask) {
                    const int pp = p0 + __ffsll((long long)hmask) - 1;
                    hmask &= hmask - 1;
                    const float *c = coords + ((size_t)rr * P + pp) * 2;
                    float X, Y;
                    point_frame(b, c[0], c[1], X, Y);
                    const PointTaps t = point_taps(X * scale, Y * scale, W, H);
                    if (!loaded) {
                        for (int cell = 0; cell < PB_CELLS; ++cell) {
                            const int cy = py0 + cell / PB_W, cx = px0 + cell % PB_W;
                            if (cy < ye && cx < xe)
                                for (int q = lane; q < C4; q += 64) acc[cell * C4 + q] = ld4(gm + ((size_t)cy * W + cx) * C + 4 * q);
                        }
                        loaded = true;
                    }
                    const float *g = g_in + ((size_t)rr * P + pp) * ld;
                    for (int q = lane; q < C4; q += 64) {
                        const float4 gv = ld4(g + 4 * q);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int x = t.x0 + (k & 1), y = t.y0 + (k >> 1);
                            if (x < px0 || x >= xe || y < py0 || y >= ye) continue;
                            const float w = k == 0 ? t.w00 : k == 1 ? t.w01 : k == 2 ? t.w10 : t.w11;
                            float4 a = acc[((y - py0) * PB_W + (x - px0)) * C4 + q];
                            a.x += w * gv.x; a.y += w * gv.y; a.z += w * gv.z; a.w += w * gv.w;
                            acc[((y - py0) * PB_W + (x - px0)) * C4 + q] = a;
                        }
                    }
                }
            }
        }
    }
    if (!loaded) return;
    for (int cell = 0; cell < PB_CELLS; ++cell) {
        const int cy = py0 + cell / PB_W, cx = px0 + cell % PB_W;
        if (cy < ye && cx < xe)
            for (int q = lane; q < C4; q += 64) st4(gm + ((size_t)cy * W + cx) * C + 4 * q, acc[cell * C4 + q]);
    }
}

// ---- concatenation of the coarse channels in front of fc2, fc3 and the predictor ----------------------------------------------------------
// out (n, cin_p) = [h (n, Ch) | x0 (n, ld0)[c0 : c0 + n_coarse] | zeros]: a thread per float4
__global__ __launch_bounds__(NT) void k_point_concat_fwd(const float *__restrict__ h, int Ch4, const float *__restrict__ x0, int ld0, int c0,
                                                         int n_coarse, size_t n4, int cin4, float *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
        const int q = (int)(i % cin4);
        const size_t pt = i / cin4;
        float4 o = f4(0.f);
        if (q < Ch4) {
            o = ld4(h + (pt * Ch4 + q) * 4);
        } else {
            const int c = 4 * (q - Ch4);
            if (c < n_coarse) {
                o = ld4(x0 + pt * ld0 + c0 + c);
                if (c + 1 >= n_coarse) o.y = 0.f;
                if (c + 2 >= n_coarse) o.z = 0.f;
                if (c + 3 >= n_coarse) o.w = 0.f;
            }
        }
        st4(out + i * 4, o);
    }
}

// g_h (n, Ch) = g_in (n, cin_p)[:, :Ch]
__global__ __launch_bounds__(NT) void k_point_concat_bwd(const float *__restrict__ g_in, int cin4, int Ch4, size_t n4, float *__restrict__ g_h) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT)
        st4(g_h + i * 4, ld4(g_in + ((i / Ch4) * cin4 + i % Ch4) * 4));
}

// ---- soft targets -------------------------------------------------------------------------------------------------------------------------
// A thread per (row, point): the assigned ground-truth mask, read as 1.0 where the byte is nonzero, sampled at the point's frame position.
// Live rule of mrcnn_maskiou_target: slot below n_pos[i], label > 0, assignment below min(G, n_gt[i]); every other row gets -1.
__global__ __launch_bounds__(NT) void k_point_target(const unsigned char *__restrict__ masks, int G, int H, int W,
                                                     const int32_t *__restrict__ n_gt, const float *__restrict__ rois,
                                                     const int32_t *__restrict__ gt_assign, const int32_t *__restrict__ label,
                                                     const int32_t *__restrict__ n_pos, int n_sample, int rows,
                                                     const float *__restrict__ coords, int P, long long n, float *__restrict__ target) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const int r = (int)(i / P), img = r / rows, j = r % rows;
        const int g = gt_assign[(size_t)img * n_sample + j];
        float t = -1.f;
        if (j < n_pos[img] && label[r] > 0 && g >= 0 && g < G && g < n_gt[img]) {
            const Roi5 b = load_roi(rois, r);
            float X, Y;
            point_frame(b, coords[i * 2], coords[i * 2 + 1], X, Y);
            const unsigned char *m = masks + ((size_t)img * G + g) * (size_t)H * W;
            t = point_sample(point_taps(X, Y, W, H), W, H, [&](int y, int x) { return m[(size_t)y * W + x] ? 1.f : 0.f; });
        }
        target[i] = t;
    }
}

// ---- loss ---------------------------------------------------------------------------------------------------------------------------------
// PHASE 0: (weight * sum of BCE, count) over the points with target >= 0 whose row has a channel.  PHASE 1: every element of gx (n, ld).
template <int PHASE>
__global__ __launch_bounds__(NT) void k_point_bce(const float *__restrict__ pred, int ld, int n_channels, const float *__restrict__ target,
                                                  const int32_t *__restrict__ label, int label_base, long long n, int P, float weight,
                                                  float *__restrict__ part, const float *__restrict__ norm, float *__restrict__ gx) {
    if (PHASE == 0) {
        float ls = 0.f, cnt = 0.f;
        for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
            const int ch = label[i / P] - label_base;
            const float t = target[i];
            if (!(t >= 0.f) || ch < 0 || ch >= n_channels) continue;
            const float v = pred[(size_t)i * ld + ch];
            ls += bce_logit1(v, t);
            cnt += 1.f;
        }
        block_partial(ls * weight, cnt, part);
    } else {
        const float scale = weight * (1.0f / norm[1]);
        for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n * ld; e += (long long)gridDim.x * NT) {
            const long long i = e / ld;
            const int c = (int)(e % ld), ch = label[i / P] - label_base;
            const float t = target[i];
            gx[e] = (t >= 0.f && ch >= 0 && ch < n_channels && c == ch) ? (sigmoid1(pred[e]) - t) * scale : 0.f;
        }
    }
}

// ---- subdivision --------------------------------------------------------------------------------------------------------------------------
constexpr int SD_T = 1024;              // threads of the one workgroup per detection
constexpr int SD_MAX_CELLS = 112 * 112; // the upsampled grid the LDS holds

// exclusive prefix sum of one int per thread over the SD_T threads, in thread order; total = the sum
__device__ __forceinline__ int sd_scan(int v, int *wtot, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(inc, o);
        if (lane >= o) inc += n;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < SD_T / 64; ++w) {
        if (w < wave) base += wtot[w];
        tot += wtot[w];
    }
    total = tot;
    return base + inc - v;
}

// One workgroup per detection.  (1) up[y][x] = the grid's channel at the centre ((x + 0.5) / 2, (y + 0.5) / 2) with clamped taps, kept in
// LDS and written out.  (2) the n_sel-th smallest |value| by a radix select over its float bits, 8 bits a pass (integer LDS atomics).
// (3) the cells below it, and the first of those equal to it in flat-index order, compacted in ascending flat index: every thread owns a
// contiguous run of cells and two prefix sums place them.  index (D, n_sel) flat cell indices, coords (D, n_sel, 2) their centres.
__global__ __launch_bounds__(SD_T) void k_point_subdivide(const float *__restrict__ grid, int S, int ld, int n_channels,
                                                          const int32_t *__restrict__ label, int n_sel, float *__restrict__ up,
                                                          int32_t *__restrict__ index, float *__restrict__ coords) {
    __shared__ float sv[SD_MAX_CELLS];
    __shared__ int hist[256];
    __shared__ int wtot[SD_T / 64];
    __shared__ unsigned s_prefix;
    __shared__ int s_k;
    const int d = blockIdx.x, S2 = 2 * S, cells = S2 * S2;
    int ch = label ? label[d] : 0;
    if (ch < 0 || ch >= n_channels) ch = 0;
    const float *g = grid + (size_t)d * S * S * ld + ch;
    for (int i = threadIdx.x; i < cells; i += SD_T) {
        const int y = i / S2, x = i % S2;
        const PointTaps t = point_taps(((float)x + 0.5f) * 0.5f, ((float)y + 0.5f) * 0.5f, S, S);
        const int xa = max(t.x0, 0), xb = min(t.x0 + 1, S - 1), ya = max(t.y0, 0), yb = min(t.y0 + 1, S - 1);
        float s = t.w00 * g[((size_t)ya * S + xa) * ld];
        s += t.w01 * g[((size_t)ya * S + xb) * ld];
        s += t.w10 * g[((size_t)yb * S + xa) * ld];
        s += t.w11 * g[((size_t)yb * S + xb) * ld];
        sv[i] = s;
        up[(size_t)d * cells + i] = s;
    }
    if (threadIdx.x == 0) { s_prefix = 0u; s_k = n_sel; }
    unsigned mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        const unsigned prefix = s_prefix;
        for (int i = threadIdx.x; i < cells; i += SD_T) {
            const unsigned k = __float_as_uint(fabsf(sv[i]));
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int k = s_k, b = 0;
            while (b < 255 && hist[b] < k) { k -= hist[b]; ++b; }
            s_k = k;
            s_prefix = prefix | ((unsigned)b << shift);
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned T = s_prefix;
    const int need = s_k;                   // cells equal to T that are taken, the lowest flat indices first
    const int chunk = (cells + SD_T - 1) / SD_T;
    const int i0 = min((int)threadIdx.x * chunk, cells), i1 = min(i0 + chunk, cells);
    int eq = 0;
    for (int i = i0; i < i1; ++i) eq += __float_as_uint(fabsf(sv[i])) == T;
    int total;
    int eq_before = sd_scan(eq, wtot, total);
    int cnt = 0;
    {
        int e = eq_before;
        for (int i = i0; i < i1; ++i) {
            const unsigned k = __float_as_uint(fabsf(sv[i]));
            cnt += k < T || (k == T && e++ < need);
        }
    }
    int pos = sd_scan(cnt, wtot, total);
    int e = eq_before;
    for (int i = i0; i < i1; ++i) {
        const unsigned k = __float_as_uint(fabsf(sv[i]));
        if ((k < T || (k == T && e++ < need)) && pos < n_sel) {
            index[(size_t)d * n_sel + pos] = i;
            float *c = coords + ((size_t)d * n_sel + pos) * 2;
            c[0] = ((float)(i % S2) + 0.5f) / (float)S2;
            c[1] = ((float)(i / S2) + 0.5f) / (float)S2;
            ++pos;
        }
    }
}

// grid (D, cells)[d, index[d, j]] = pred (D * n_sel, ld)[d * n_sel + j, label[d]]
__global__ __launch_bounds__(NT) void k_point_scatter(const float *__restrict__ pred, int ld, int n_channels, const int32_t *__restrict__ label,
                                                      const int32_t *__restrict__ index, long long n, int n_sel, int cells,
                                                      float *__restrict__ grid) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const int d = (int)(i / n_sel);
        int ch = label ? label[d] : 0;
        if (ch < 0 || ch >= n_channels) ch = 0;
        const int cell = index[i];
        if (cell >= 0 && cell < cells) grid[(size_t)d * cells + cell] = pred[(size_t)i * ld + ch];
    }
}

int ew_blocks(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + NT - 1) / NT, 65535)); }

}  // namespace

extern "C" int mrcnn_point_train_coords(const uint32_t *keys, int n_keys, const float *coarse, int S0, int Cp, int n_channels,
                                        const int32_t *label, int label_base, int rows, int P, int n_cand, int n_imp, float *coords,
                                        void *stream) {
    if (rows < 0 || S0 <= 0 || Cp <= 0 || P <= 0 || n_cand <= 0 || n_imp < 0 || n_imp > P || n_imp > n_cand || n_keys <= 0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_train_coords: bad sizes (S0, Cp, P, n_cand, n_keys > 0; 0 <= n_imp <= min(P, n_cand))");
    if (n_channels <= 0 || n_channels > Cp)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_train_coords: %d label channels outside the %d of the coarse logits", n_channels, Cp);
    if (n_cand > PT_MAX_CAND) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "point_train_coords: %d candidates per row (at most %d)", n_cand, PT_MAX_CAND);
    if ((long long)n_keys < 2ll * n_cand + 2ll * (P - n_imp))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_train_coords: %d keys per row, %lld needed", n_keys, 2ll * n_cand + 2ll * (P - n_imp));
    if (rows == 0) return 0;
    if (!keys || !coarse || !label || !coords) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_train_coords: null pointer");
    int n2 = 2;
    while (n2 < n_cand) n2 <<= 1;
    hipLaunchKernelGGL(k_point_train_coords, dim3(rows), dim3(NT), 0, (hipStream_t)stream, keys, n_keys, coarse, S0, Cp, n_channels, label,
                       label_base, P, n_cand, n_imp, n2, coords);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_point_features_fwd(const float *coords, const float *rois_xy5, const float *map, int N, int H, int W, int C, float scale,
                                        const float *coarse, int S0, int Cp, int n_channels, int rows, int P, int cin_p, float *out,
                                        void *stream) {
    if (rows < 0 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || S0 <= 0 || Cp <= 0 || P <= 0 || cin_p <= 0 || (C % 4) || (Cp % 4) || (cin_p % 4) ||
        !(scale > 0.f))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_features_fwd: bad sizes (C, Cp and cin_p multiples of 4, scale > 0)");
    if (n_channels <= 0 || n_channels > Cp || cin_p < C + n_channels)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_features_fwd: %d coarse channels outside the %d of the logits or the %d - %d of the input",
                               n_channels, Cp, cin_p, C);
    if (rows == 0) return 0;
    if (!coords || !rois_xy5 || !map || !coarse || !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_features_fwd: null pointer");
    const long long n_points = (long long)rows * P;
    hipLaunchKernelGGL(k_point_features_fwd, dim3(ew_blocks(n_points * 64)), dim3(NT), 0, (hipStream_t)stream, coords, rois_xy5, map, N, H, W, C,
                       scale, coarse, S0, Cp, n_channels, n_points, P, cin_p, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_point_features_bwd(const float *g_in, int ld, const float *coords, const float *rois_xy5, int rows, int P, float scale,
                                        float *g_map, int N, int H, int W, int C, void *stream) {
    if (rows < 0 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || P <= 0 || ld <= 0 || (C % 4) || (ld % 4) || ld < C || !(scale > 0.f))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_features_bwd: bad sizes (C and ld multiples of 4, ld >= C, scale > 0)");
    const size_t lds = (size_t)PB_WAVES * PB_CELLS * C * sizeof(float);
    if (lds > 64 * 1024) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "point_features_bwd: %d channels (at most %d)", C, 64 * 1024 / (PB_WAVES * PB_CELLS * 4));
    if (rows == 0) return 0;
    if (!g_in || !coords || !rois_xy5 || !g_map) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_features_bwd: null pointer");
    const int tx = mrcnn::cdiv(W, PB_W), ty = mrcnn::cdiv(H, PB_H);
    const long long n_patches = (long long)N * tx * ty;
    if (n_patches > (1ll << 31) - 1) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "point_features_bwd: map too large");
    hipLaunchKernelGGL(k_point_features_bwd, dim3(mrcnn::cdiv(n_patches, PB_WAVES)), dim3(NT), lds, (hipStream_t)stream, g_in, ld, coords,
                       rois_xy5, rows, P, scale, g_map, H, W, C, tx, ty, n_patches);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_point_concat_fwd(const float *h, int Ch, const float *x0, int ld0, int c0, int n_coarse, long long n_points, int cin_p,
                                      float *out, void *stream) {
    if (n_points < 0 || Ch <= 0 || ld0 <= 0 || c0 < 0 || n_coarse <= 0 || cin_p <= 0 || (Ch % 4) || (ld0 % 4) || (c0 % 4) || (cin_p % 4))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_concat_fwd: bad sizes (Ch, ld0, c0 and cin_p multiples of 4)");
    if (cin_p < Ch + n_coarse || (c0 + n_coarse + 3) / 4 * 4 > ld0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_concat_fwd: %d coarse channels outside the input's %d or the output's %d - %d", n_coarse,
                               ld0, cin_p, Ch);
    if (n_points == 0) return 0;
    if (!h || !x0 || !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_concat_fwd: null pointer");
    const size_t n4 = (size_t)n_points * (cin_p / 4);
    hipLaunchKernelGGL(k_point_concat_fwd, dim3(ew_blocks((long long)n4)), dim3(NT), 0, (hipStream_t)stream, h, Ch / 4, x0, ld0, c0, n_coarse, n4,
                       cin_p / 4, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_point_concat_bwd(const float *g_in, int cin_p, int Ch, long long n_points, float *g_h, void *stream) {
    if (n_points < 0 || Ch <= 0 || cin_p <= 0 || (Ch % 4) || (cin_p % 4) || cin_p < Ch)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_concat_bwd: bad sizes (Ch and cin_p multiples of 4, cin_p >= Ch)");
    if (n_points == 0) return 0;
    if (!g_in || !g_h) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_concat_bwd: null pointer");
    const size_t n4 = (size_t)n_points * (Ch / 4);
    hipLaunchKernelGGL(k_point_concat_bwd, dim3(ew_blocks((long long)n4)), dim3(NT), 0, (hipStream_t)stream, g_in, cin_p / 4, Ch / 4, n4, g_h);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_point_target(const uint8_t *masks, int N, int G, int H, int W, const int32_t *n_gt, const float *rois_xy5,
                                  const int32_t *gt_assign, const int32_t *label, const int32_t *n_pos, int n_sample, int rows,
                                  const float *coords, int P, float *target, void *stream) {
    if (N <= 0 || G <= 0 || H <= 0 || W <= 0 || n_sample <= 0 || rows < 0 || rows > n_sample || P <= 0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_target: bad sizes (N, G, H, W, n_sample, P > 0; 0 <= rows <= n_sample)");
    if (rows == 0) return 0;
    if (!masks || !n_gt || !rois_xy5 || !gt_assign || !label || !n_pos || !coords || !target)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_target: null pointer");
    const long long n = (long long)N * rows * P;
    hipLaunchKernelGGL(k_point_target, dim3(ew_blocks(n)), dim3(NT), 0, (hipStream_t)stream, masks, G, H, W, n_gt, rois_xy5, gt_assign, label,
                       n_pos, n_sample, rows, coords, P, n, target);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_point_bce(const float *pred, int ld, int n_channels, const float *target, const int32_t *label, int label_base, int rows,
                               int P, float weight, float *loss_out, float *gx, void *ws, size_t ws_bytes, void *stream) {
    if (rows < 0 || ld <= 0 || P <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_bce: bad sizes");
    if (n_channels <= 0 || n_channels > ld)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_bce: %d label channels outside the %d columns of pred", n_channels, ld);
    if (!(weight > 0.f) || weight > 3.0e38f) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_bce: weight must be a finite number above 0");
    if ((rows > 0 && (!pred || !target || !label)) || !loss_out || !ws) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_bce: null pointer");
    if (ws_bytes < mrcnn_loss_workspace_bytes()) return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "point_bce: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)ws;
    const long long n = (long long)rows * P;
    const int nb = grid_for(n);
    hipLaunchKernelGGL(k_point_bce<0>, dim3(nb), dim3(NT), 0, st, pred, ld, n_channels, target, label, label_base, n, P, weight, part, nullptr,
                       nullptr);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, st, part, nb, loss_out);
    MRCNN_LAUNCH_CHECK();
    if (gx && rows > 0) {
        hipLaunchKernelGGL(k_point_bce<1>, dim3(grid_for(n * ld)), dim3(NT), 0, st, pred, ld, n_channels, target, label, label_base, n, P, weight,
                           part, loss_out, gx);
        MRCNN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mrcnn_point_subdivide(const float *grid, int D, int S, int ld, int n_channels, const int32_t *label, int n_sel, float *up,
                                     int32_t *index, float *coords, void *stream) {
    if (D < 0 || S <= 0 || ld <= 0 || n_sel <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_subdivide: bad sizes");
    if (n_channels <= 0 || n_channels > ld)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_subdivide: %d label channels outside the %d of the grid", n_channels, ld);
    if (4ll * S * S > SD_MAX_CELLS) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "point_subdivide: a %d x %d grid (at most 56 x 56)", S, S);
    if (n_sel > 4 * S * S) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_subdivide: %d cells of %d selected", n_sel, 4 * S * S);
    if (D == 0) return 0;
    if (!grid || !up || !index || !coords) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_subdivide: null pointer");
    hipLaunchKernelGGL(k_point_subdivide, dim3(D), dim3(SD_T), 0, (hipStream_t)stream, grid, S, ld, n_channels, label, n_sel, up, index, coords);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_point_scatter(const float *pred, int ld, int n_channels, const int32_t *label, const int32_t *index, int D, int n_sel,
                                   int cells, float *grid, void *stream) {
    if (D < 0 || ld <= 0 || n_sel <= 0 || cells <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_scatter: bad sizes");
    if (n_channels <= 0 || n_channels > ld)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "point_scatter: %d label channels outside the %d columns of pred", n_channels, ld);
    if (D == 0) return 0;
    if (!pred || !index || !grid) return mrcnn::fail_arg(MRCNN_E_INVALID, "point_scatter: null pointer");
    const long long n = (long long)D * n_sel;
    hipLaunchKernelGGL(k_point_scatter, dim3(ew_blocks(n)), dim3(NT), 0, (hipStream_t)stream, pred, ld, n_channels, label, index, n, n_sel, cells,
                       grid);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
