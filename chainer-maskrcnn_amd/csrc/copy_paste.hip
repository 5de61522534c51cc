// Simple Copy-Paste on a large-scale-jitter batch (dataset/augment.py copy_paste_batch is the rule).  Example n of the
// batch receives from its partner p = (n + 1) % N: the partner's valid rows (label >= 0) that are offered - sel[p][gather[p][j]] != 0,
// the offer keyed by the ORIGINAL instance index the LSJ gather table carries - are pasted over n when receive[n] is set.  Every kernel
// reads the pre-paste batch and writes new tensors; the arithmetic is selection, AND-NOT and integer max, so every output is exact.
//   k_cp_compose   thread = 16 consecutive x of one row of one example: ORs the picked partner planes into an (N,H,W) alpha plane
//                  (0xFF where pasted) and writes out = alpha ? imgs[p] : imgs[n] on 3 channels.  The alpha plane is what the later
//                  passes read instead of the G partner planes.
//   k_cp_reduce    augment.hip's k_mask_crop_reduce scheme over the G + G candidate rows (a block takes own row g, then partner row
//                  g: the grid's y extent stays G <= 65535): own row r as mask & ~alpha, partner row j unchanged; (H - y, W - x,
//                  y + 1, x + 1) max-reduced by wave shuffles, LDS across the 4 waves and at most 4 integer atomicMax per block and
//                  candidate into a zero-filled (N,2G,4) workspace.  Rows that are no candidates are left at once.
//   k_cp_finalize  one wave per example: ballot prefix count over the candidates in order; boxes, labels and the source table
//                  (r < G: own row r minus alpha; G + j: partner row j; -1: a zero plane), trailing rows included.
//   k_cp_masks     output plane k from its source code, written once, padding included.
// Rows whose 16-byte chunks are aligned (W % 16 == 0 and aligned tensors: `vec`) move as uint4 / float4; every other shape takes the
// byte / scalar path with a ragged last thread - no access leaves its row.
#include "common.h"

namespace {

constexpr int NT = 256;

// 0xFF in every byte of w that is non-zero, 0x00 elsewhere
__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {
    const unsigned t = (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
    return (t >> 7) * 0xFFu;
}

// 16 bytes of a row at x0 as 4 words (little-endian byte order, as a uint4 load gives them); bytes at x >= W are 0
__device__ __forceinline__ void load16(const uint8_t *__restrict__ row, int x0, int W, bool vec, unsigned (&v)[4]) {
    if (vec) {
        const uint4 q = *reinterpret_cast<const uint4 *>(row + x0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = v[1] = v[2] = v[3] = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (x0 + j < W) v[j >> 2] |= (unsigned)row[x0 + j] << (8 * (j & 3));
    }
}

__device__ __forceinline__ void store16(uint8_t *__restrict__ row, int x0, int W, bool vec, const unsigned (&v)[4]) {
    if (vec) {
        *reinterpret_cast<uint4 *>(row + x0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (x0 + j < W) row[x0 + j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
    }
}

// Is row j of partner p pasted onto its receiver?  (receive is the caller's test.)  Uniform per (p, j).
__device__ __forceinline__ bool offered(const int32_t *__restrict__ labels, const int32_t *__restrict__ gather,
                                        const uint8_t *__restrict__ sel, int p, int j, int G, int Gin) {
    if (labels[(size_t)p * G + j] < 0) return false;
    const int g = gather[(size_t)p * G + j];
    return g >= 0 && g < Gin && sel[(size_t)p * Gin + g] != 0;
}

// grid (cdiv(H * wq, NT), N); wq = cdiv(W, 16)
__global__ __launch_bounds__(NT) void k_cp_compose(const float *__restrict__ imgs, const uint8_t *__restrict__ masks,
                                                   const int32_t *__restrict__ labels, const int32_t *__restrict__ gather,
                                                   const uint8_t *__restrict__ sel, const uint8_t *__restrict__ receive,
                                                   float *__restrict__ out, uint8_t *__restrict__ alpha, int N, int G, int Gin, int H,
                                                   int W, int wq, int vec) {
    __shared__ int picked[NT];
    const int n = blockIdx.y, p = (n + 1) % N;
    const int i = blockIdx.x * NT + threadIdx.x;
    const bool active = i < H * wq;                          // (idle threads of the last block stay for the barriers)
    const int y = active ? i / wq : 0, x0 = active ? (i - y * wq) * 16 : 0;
    unsigned a[4] = {0u, 0u, 0u, 0u};
    if (receive[n]) {                                        // block-uniform
        for (int base = 0; base < G; base += NT) {
            const int j = base + threadIdx.x;
            picked[threadIdx.x] = j < G && offered(labels, gather, sel, p, j, G, Gin);
            __syncthreads();
            const int m = min(NT, G - base);
            for (int k = 0; k < m; ++k) {
                if (!picked[k] || !active) continue;
                unsigned w[4];
                load16(masks + (((size_t)p * G + base + k) * H + y) * W, x0, W, vec, w);
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] |= nonzero_bytes(w[q]);
            }
            __syncthreads();
        }
    }
    if (!active) return;
    store16(alpha + ((size_t)n * H + y) * W, x0, W, vec, a);
    const size_t plane = (size_t)H * W;
    const size_t at = (size_t)y * W + x0;
    const bool any = (a[0] | a[1] | a[2] | a[3]) != 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *own = imgs + ((size_t)n * 3 + c) * plane + at;
        const float *par = imgs + ((size_t)p * 3 + c) * plane + at;
        float *o = out + ((size_t)n * 3 + c) * plane + at;
        if (vec) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 v = ld4(own + 4 * q);
                if (a[q]) {
                    const float4 u = ld4(par + 4 * q);
                    if (a[q] & 0xFFu) v.x = u.x;
                    if (a[q] & 0xFF00u) v.y = u.y;
                    if (a[q] & 0xFF0000u) v.z = u.z;
                    if (a[q] & 0xFF000000u) v.w = u.w;
                }
                *reinterpret_cast<float4 *>(o + 4 * q) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (x0 + j < W) o[j] = (any && ((a[j >> 2] >> (8 * (j & 3))) & 0xFFu)) ? par[j] : own[j];
        }
    }
}

// Candidate c of example n: c < G its own row c (valid: label >= 0), c >= G the partner's row c - G (picked).  Block-uniform.
__device__ __forceinline__ bool candidate(const int32_t *__restrict__ labels, const int32_t *__restrict__ gather,
                                          const uint8_t *__restrict__ sel, const uint8_t *__restrict__ receive, int n, int p, int c, int G,
                                          int Gin) {
    if (c < G) return labels[(size_t)n * G + c] >= 0;
    return receive[n] && offered(labels, gather, sel, p, c - G, G, Gin);
}

// 16 bytes of what candidate / source code c of example n keeps at (y, x0): own row minus alpha, or the partner's row as it is
__device__ __forceinline__ void candidate16(const uint8_t *__restrict__ masks, const uint8_t *__restrict__ alpha, int n, int p, int c,
                                            int G, int H, int W, int y, int x0, bool vec, unsigned (&w)[4]) {
    if (c < G) {
        unsigned a[4];
        load16(masks + (((size_t)n * G + c) * H + y) * W, x0, W, vec, w);
        load16(alpha + ((size_t)n * H + y) * W, x0, W, vec, a);
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] &= ~a[q];
    } else {
        load16(masks + (((size_t)p * G + (c - G)) * H + y) * W, x0, W, vec, w);
    }
}

// grid (cdiv(H * wq, NT), G, N); the block of row g reduces candidate g (own row g), then candidate G + g (partner row g).  ws (N,2G,4)
// int32, zero-filled before the launch: per candidate the maxima of (H - y, W - x, y + 1, x + 1) over its remaining pixels - all four
// >= 1 where one remains, so 0 means "no pixel" (k_mask_crop_reduce's encoding).
__global__ __launch_bounds__(NT) void k_cp_reduce(const uint8_t *__restrict__ masks, const uint8_t *__restrict__ alpha,
                                                  const int32_t *__restrict__ labels, const int32_t *__restrict__ gather,
                                                  const uint8_t *__restrict__ sel, const uint8_t *__restrict__ receive,
                                                  int32_t *__restrict__ ws, int N, int G, int Gin, int H, int W, int wq, int vec) {
    __shared__ int part[NT / kWave][4];
    const int n = blockIdx.z, p = (n + 1) % N;
    const int i = blockIdx.x * NT + threadIdx.x;
    const int y = i / wq, x0 = (i - y * wq) * 16;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (int c = blockIdx.y; c < 2 * G; c += G) {
        if (!candidate(labels, gather, sel, receive, n, p, c, G, Gin)) continue;      // block-uniform
        int v[4] = {0, 0, 0, 0};
        if (i < H * wq) {
            unsigned w[4];
            candidate16(masks, alpha, n, p, c, G, H, W, y, x0, vec, w);
            int lo = -1, hi = -1;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) {
                    if (lo < 0) lo = j;
                    hi = j;
                }
            if (lo >= 0) {
                v[0] = H - y; v[1] = W - (x0 + lo); v[2] = y + 1; v[3] = x0 + hi + 1;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) v[k] = max(v[k], __shfl_xor(v[k], off, kWave));
        __syncthreads();                                     // (the partials of the first candidate have been read)
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) part[wave][k] = v[k];
        __syncthreads();
        if (threadIdx.x < 4) {
            int m = 0;
#pragma unroll
            for (int q = 0; q < NT / kWave; ++q) m = max(m, part[q][threadIdx.x]);
            if (m > 0) atomicMax(&ws[((size_t)n * 2 * G + c) * 4 + threadIdx.x], m);
        }
    }
}

// grid N, one wave per example.  The candidates that kept a pixel, in candidate order, become output rows 0, 1, ... (those past G_out
// are dropped): tight box, label and source code; the rows behind them get a zero box, label -1 and source -1.
__global__ __launch_bounds__(kWave) void k_cp_finalize(const int32_t *__restrict__ ws, const int32_t *__restrict__ labels,
                                                       float *__restrict__ bboxes, int32_t *__restrict__ labels_out,
                                                       int32_t *__restrict__ source, int N, int G, int G_out, int H, int W) {
    const int n = blockIdx.x, lane = threadIdx.x, p = (n + 1) % N;
    int kept = 0;
    for (int base = 0; base < 2 * G; base += kWave) {                  // (uniform bounds: every lane reaches the ballot)
        const int c = base + lane;
        int4 r = make_int4(0, 0, 0, 0);
        if (c < 2 * G) r = reinterpret_cast<const int4 *>(ws)[(size_t)n * 2 * G + c];
        const bool keep = r.x > 0;
        const unsigned long long m = __ballot(keep);
        const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < G_out) {
            const size_t o = (size_t)n * G_out + pos;
            reinterpret_cast<float4 *>(bboxes)[o] = make_float4((float)(H - r.x), (float)(W - r.y), (float)r.z, (float)r.w);
            labels_out[o] = c < G ? labels[(size_t)n * G + c] : labels[(size_t)p * G + (c - G)];
            source[o] = c;
        }
        kept += __popcll(m);
    }
    for (int j = min(kept, G_out) + lane; j < G_out; j += kWave) {
        const size_t o = (size_t)n * G_out + j;
        reinterpret_cast<float4 *>(bboxes)[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        labels_out[o] = -1;
        source[o] = -1;
    }
}

// grid (cdiv(H * wq, NT), G_out, N)
__global__ __launch_bounds__(NT) void k_cp_masks(const uint8_t *__restrict__ masks, const uint8_t *__restrict__ alpha,
                                                 const int32_t *__restrict__ source, uint8_t *__restrict__ out, int N, int G, int G_out,
                                                 int H, int W, int wq, int vec) {
    const int n = blockIdx.z, k = blockIdx.y, p = (n + 1) % N;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= H * wq) return;
    const int y = i / wq, x0 = (i - y * wq) * 16;
    const int c = source[(size_t)n * G_out + k];
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (c >= 0 && c < 2 * G) candidate16(masks, alpha, n, p, c, G, H, W, y, x0, vec, w);
    store16(out + (((size_t)n * G_out + k) * H + y) * W, x0, W, vec, w);
}

int check_sizes(const char *who, int N, int G, int Gin, int H, int W) {
    if (N < 2 || N > MRCNN_RESIZE_BATCH_MAX)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: N = %d outside 2..%d (an example receives from its neighbour)", who, N,
                               MRCNN_RESIZE_BATCH_MAX);
    if (G < 1 || G > 65535) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: G = %d outside 1..65535", who, G);
    if (Gin < 1 || Gin > 65535) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: Gin = %d outside 1..65535", who, Gin);
    if (H <= 0 || W <= 0 || (long long)H * ((long long)W + 15) > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad size H x W = %d x %d", who, H, W);
    return 0;
}

inline bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

extern "C" int mrcnn_copy_paste_image_f32(const float *imgs, const unsigned char *masks, const int32_t *labels, const int32_t *gather,
                                          const unsigned char *sel, const unsigned char *receive, int N, int G, int Gin, int H, int W,
                                          float *out_imgs, unsigned char *alpha, void *stream) {
    const char *who = "copy_paste_image";
    if (!imgs) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null imgs", who);
    if (!masks) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null masks", who);
    if (!labels) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null labels", who);
    if (!gather) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gather", who);
    if (!sel) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null sel", who);
    if (!receive) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null receive", who);
    if (!out_imgs) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null out_imgs", who);
    if (!alpha) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null alpha", who);
    if (int e = check_sizes(who, N, G, Gin, H, W)) return e;
    if (!aligned16(out_imgs)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: out_imgs not 16-byte aligned", who);
    if (!aligned16(alpha)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: alpha not 16-byte aligned", who);
    const int wq = (W + 15) / 16;
    const int vec = (W % 16 == 0) && aligned16(imgs) && aligned16(masks);
    hipLaunchKernelGGL(k_cp_compose, dim3(mrcnn::cdiv((long long)H * wq, NT), N), dim3(NT), 0, (hipStream_t)stream, imgs, masks, labels,
                       gather, sel, receive, out_imgs, alpha, N, G, Gin, H, W, wq, vec);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_copy_paste_masks_u8(const unsigned char *masks, const unsigned char *alpha, const int32_t *labels,
                                         const int32_t *gather, const unsigned char *sel, const unsigned char *receive, int N, int G,
                                         int Gin, int G_out, int H, int W, unsigned char *out_masks, float *bboxes, int32_t *labels_out,
                                         int32_t *source, int32_t *ws, void *stream) {
    const char *who = "copy_paste_masks";
    if (!masks) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null masks", who);
    if (!alpha) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null alpha", who);
    if (!labels) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null labels", who);
    if (!gather) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null gather", who);
    if (!sel) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null sel", who);
    if (!receive) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null receive", who);
    if (!out_masks) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null out_masks", who);
    if (!bboxes) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null bboxes", who);
    if (!labels_out) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null labels_out", who);
    if (!source) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null source", who);
    if (!ws) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null ws", who);
    if (int e = check_sizes(who, N, G, Gin, H, W)) return e;
    if (G_out < 1 || G_out > 65535) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: G_out = %d outside 1..65535", who, G_out);
    if (!aligned16(out_masks)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: out_masks not 16-byte aligned", who);
    if (!aligned16(bboxes)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bboxes not 16-byte aligned", who);
    if (!aligned16(ws)) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: ws not 16-byte aligned", who);
    const int wq = (W + 15) / 16;
    const int vec = (W % 16 == 0) && aligned16(masks) && aligned16(alpha);
    hipStream_t st = (hipStream_t)stream;
    MRCNN_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)N * 2 * G * 4 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_cp_reduce, dim3(mrcnn::cdiv((long long)H * wq, NT), G, N), dim3(NT), 0, st, masks, alpha, labels, gather, sel,
                       receive, ws, N, G, Gin, H, W, wq, vec);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cp_finalize, dim3(N), dim3(kWave), 0, st, ws, labels, bboxes, labels_out, source, N, G, G_out, H, W);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cp_masks, dim3(mrcnn::cdiv((long long)H * wq, NT), G_out, N), dim3(NT), 0, st, masks, alpha, source, out_masks, N,
                       G, G_out, H, W, wq, vec);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
