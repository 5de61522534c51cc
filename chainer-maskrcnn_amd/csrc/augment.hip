// Batched training resizes with an optional horizontal flip (dataset/loader.py BatchLoader(augment=...)).
// The device side of Transform(hflip(example)) for a whole batch: the raw uint8 images (and masks) of the N examples arrive packed in
// one buffer, each example's geometry in a small descriptor table passed by value, and ONE launch per tensor writes the whole
// zero-padded batch tensor, padding included, so the tensor needs no memset first.
//   image: thread = 4 consecutive x of one output row of one example, all 3 channels -> three 16-byte stores
//   masks: thread = 16 consecutive x of one output row of one instance of one example -> one 16-byte store
// Taps: resize_common.h (the same linear_tap / nearest_tap as nn.hip's per-image kernels).  A flipped example computes the taps as
// usual and reads source column s as W-1-s: bit-identical to resizing src[..., ::-1].
// Memory-bound on the stores (a bs-2 1024^2 batch: 25 MB of float32 image + 1 MB per mask plane); the source reads are byte gathers
// that hit the caches (each source byte is read by ~2 neighbouring outputs per axis).
//
// Large-scale jitter runs the same two kernel bodies on a crop descriptor: the example is resized virtually to
// oh x ow and the window [y0, y0+ch) x [x0, x0+cw) of that resize lands at the top-left of the canvas - the taps of output (y, x) are
// those of (y + y0, x + x0), everything outside the window is zero.  A crop cuts instances, so two more launches precede the mask
// writer: k_mask_crop_reduce reads the cropped nearest-neighbour resize of every instance WITHOUT writing it and max-reduces its tight
// box (wave shuffles, LDS across the 4 waves, at most 4 integer atomicMax per block into a zero-filled (N, Gin, 4) workspace - integer
// max is exact and independent of arrival order), and k_mask_crop_finalize (one wave per example) packs the instances that kept a
// pixel first: boxes, labels and the gather table the mask writer reads its source instance from, so no plane is ever moved.
#include "common.h"
#include "resize_common.h"

namespace {

constexpr int NT = 256;

template <class D>
struct Descs {
    D d[MRCNN_RESIZE_BATCH_MAX];
};

// The part of the virtual oh x ow resize an example writes, at the canvas' top-left: all of it for a plain resize descriptor.
struct Window {
    int y0, x0, ch, cw;
};
__device__ __forceinline__ Window window(const mrcnn_resize_desc_t &d) { return {0, 0, d.oh, d.ow}; }
__device__ __forceinline__ Window window(const mrcnn_crop_desc_t &d) { return {d.y0, d.x0, d.ch, d.cw}; }

// grid (cdiv(dst_h * wq, NT), N); wq = cdiv(dst_w, 4)
template <class D>
__global__ __launch_bounds__(NT) void k_image_resize_batch_u8(const uint8_t *__restrict__ src, const Descs<D> ds, float *__restrict__ dst,
                                                              int dst_h, int dst_w, int wq, float div) {
    const int n = blockIdx.y;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= dst_h * wq) return;
    const D d = ds.d[n];
    const Window w = window(d);
    const int y = i / wq, x0 = (i - y * wq) * 4;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[c][j] = 0.f;
    if (y < w.ch) {
        int y0, y1;
        float b0, b1;
        linear_tap(y + w.y0, d.oh, d.H, y0, y1, b0, b1);
        const uint8_t *base = src + d.src_offset;
        const uint8_t *r0 = base + (size_t)y0 * d.W * 3, *r1 = base + (size_t)y1 * d.W * 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x < w.cw) {
                int s0, s1;
                float a0, a1;
                linear_tap(x + w.x0, d.ow, d.W, s0, s1, a0, a1);
                if (d.flip) { s0 = d.W - 1 - s0; s1 = d.W - 1 - s1; }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float top = (float)r0[s0 * 3 + c] * a0 + (float)r0[s1 * 3 + c] * a1;
                    const float bot = (float)r1[s0 * 3 + c] * a0 + (float)r1[s1 * 3 + c] * a1;
                    v[c][j] = (top * b0 + bot * b1) / div;
                }
            }
        }
    }
    const size_t plane = (size_t)dst_h * dst_w;
    float *o = dst + (size_t)n * 3 * plane + (size_t)y * dst_w + x0;
    if ((dst_w & 3) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < dst_w) o[c * plane + j] = v[c][j];
    }
}

// 16 consecutive x of row y of the window of source instance g, one byte each in 4 words (a flip mirrors the source column); 0 outside
template <class D>
__device__ __forceinline__ void mask_row16(const uint8_t *__restrict__ src, const D &d, const Window &w, int g, int y, int x0,
                                           unsigned (&v)[4]) {
    const int sy = nearest_tap(y + w.y0, d.oh, d.H);
    const uint8_t *row = src + d.src_offset + ((size_t)g * d.H + sy) * d.W;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int x = x0 + j;
        if (x < w.cw) {
            int sx = nearest_tap(x + w.x0, d.ow, d.W);
            if (d.flip) sx = d.W - 1 - sx;
            v[j >> 2] |= (unsigned)row[sx] << (8 * (j & 3));
        }
    }
}

// grid (cdiv(dst_h * wq, NT), G, N); wq = cdiv(dst_w, 16).  gather (nullable, (N,G)): output plane g reads source instance gather[n][g]
// (-1, or anything outside the example's count: a zero plane); NULL: instance g itself.
template <class D>
__global__ __launch_bounds__(NT) void k_mask_resize_batch_u8(const uint8_t *__restrict__ src, const Descs<D> ds,
                                                             const int32_t *__restrict__ gather, uint8_t *__restrict__ dst, int G, int dst_h,
                                                             int dst_w, int wq) {
    const int n = blockIdx.z, g = blockIdx.y;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= dst_h * wq) return;
    const D d = ds.d[n];
    const Window win = window(d);
    const int y = i / wq, x0 = (i - y * wq) * 16;
    const int sg = gather ? gather[n * G + g] : g;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (sg >= 0 && sg < d.count && y < win.ch) mask_row16(src, d, win, sg, y, x0, w);
    uint8_t *o = dst + (((size_t)n * G + g) * dst_h + y) * dst_w + x0;
    if ((dst_w & 15) == 0) {
        *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (x0 + j < dst_w) o[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

// Tight boxes of the cropped masks, pass 1.  grid (cdiv(dst_h * wq, NT), Gin, N), the mask writer's thread map; nothing is written but
// the workspace: ws (N,Gin,4) int32, zero-filled before the launch, receives per instance the maxima of
//   (dst_h - y, dst_w - x, y + 1, x + 1) over the set pixels (y, x) of its cropped resize,
// all four >= 1 where a pixel survives - so 0 means "no pixel", and the minima come out of the same atomicMax as the maxima.
__global__ __launch_bounds__(NT) void k_mask_crop_reduce(const uint8_t *__restrict__ src, const Descs<mrcnn_crop_desc_t> ds,
                                                         int32_t *__restrict__ ws, int Gin, int dst_h, int dst_w, int wq) {
    const int n = blockIdx.z, g = blockIdx.y;
    const mrcnn_crop_desc_t d = ds.d[n];
    const Window win = window(d);
    if (g >= d.count || (blockIdx.x * NT) / wq >= win.ch) return;      // block-uniform: no instance, or every row below the window
    const int i = blockIdx.x * NT + threadIdx.x;
    const int y = i / wq, x0 = (i - y * wq) * 16;
    int v[4] = {0, 0, 0, 0};
    if (y < win.ch) {                                                   // (rows >= ch <= dst_h take no part; i < dst_h * wq follows)
        unsigned w[4] = {0u, 0u, 0u, 0u};
        mask_row16(src, d, win, g, y, x0, w);
        int lo = -1, hi = -1;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) {
                if (lo < 0) lo = j;
                hi = j;
            }
        if (lo >= 0) {
            v[0] = dst_h - y; v[1] = dst_w - (x0 + lo); v[2] = y + 1; v[3] = x0 + hi + 1;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v[k] = max(v[k], __shfl_xor(v[k], off, kWave));
    __shared__ int part[NT / kWave][4];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) part[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        int m = 0;
#pragma unroll
        for (int q = 0; q < NT / kWave; ++q) m = max(m, part[q][threadIdx.x]);
        if (m > 0) atomicMax(&ws[((size_t)n * Gin + g) * 4 + threadIdx.x], m);
    }
}

// Pass 2: grid N, one wave per example.  The instances that kept a pixel, in their order, become output rows 0, 1, ... (rows past G are
// dropped): box (ymin, xmin, ymax + 1, xmax + 1) in canvas coordinates, the instance's label, and its index in the gather table; the
// rows behind them get a zero box, label -1 and gather -1.
__global__ __launch_bounds__(kWave) void k_mask_crop_finalize(const Descs<mrcnn_crop_desc_t> ds, const int32_t *__restrict__ ws,
                                                              const int32_t *__restrict__ labels_in, float *__restrict__ bboxes,
                                                              int32_t *__restrict__ labels, int32_t *__restrict__ gather, int Gin, int G,
                                                              int dst_h, int dst_w) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int count = ds.d[n].count;
    int kept = 0;
    for (int base = 0; base < count; base += kWave) {                  // (uniform bounds: every lane reaches the ballot)
        const int g = base + lane;
        int4 r = make_int4(0, 0, 0, 0);
        if (g < count) r = reinterpret_cast<const int4 *>(ws)[(size_t)n * Gin + g];
        const bool keep = r.x > 0;
        const unsigned long long m = __ballot(keep);
        const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < G) {
            const size_t o = (size_t)n * G + pos;
            reinterpret_cast<float4 *>(bboxes)[o] = make_float4((float)(dst_h - r.x), (float)(dst_w - r.y), (float)r.z, (float)r.w);
            labels[o] = labels_in[(size_t)n * Gin + g];
            gather[o] = g;
        }
        kept += __popcll(m);
    }
    for (int j = min(kept, G) + lane; j < G; j += kWave) {
        const size_t o = (size_t)n * G + j;
        reinterpret_cast<float4 *>(bboxes)[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        labels[o] = -1;
        gather[o] = -1;
    }
}

// Common argument checks; elem_bytes(d) = the source bytes example d reads.  Returns 0 or an MRCNN_E_* code (error already set).
template <class Bytes>
int check_batch(const char *who, const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, const void *dst,
                int dst_h, int dst_w, int G, Bytes elem_bytes, Descs<mrcnn_resize_desc_t> &out) {
    if (!desc || !dst) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null pointer", who);
    if (N < 1 || N > MRCNN_RESIZE_BATCH_MAX)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: N = %d outside 1..%d", who, N, MRCNN_RESIZE_BATCH_MAX);
    if (dst_h <= 0 || dst_w <= 0 || (long long)dst_h * (dst_w + 15) > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad output size %d x %d", who, dst_h, dst_w);
    if (reinterpret_cast<uintptr_t>(dst) & 15) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: dst not 16-byte aligned", who);
    for (int n = 0; n < N; ++n) {
        const mrcnn_resize_desc_t &d = desc[n];
        if (d.H <= 0 || d.W <= 0 || d.oh <= 0 || d.ow <= 0 || d.oh > dst_h || d.ow > dst_w || (d.flip != 0 && d.flip != 1) ||
            d.count < 0 || d.count > G || d.src_offset < 0)
            return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad descriptor %d (H %d W %d oh %d ow %d flip %d count %d offset %lld)", who, n,
                                   d.H, d.W, d.oh, d.ow, d.flip, d.count, d.src_offset);
        const unsigned long long need = elem_bytes(d);
        if (need > 0 && (!src || (unsigned long long)d.src_offset > src_bytes || need > src_bytes - (unsigned long long)d.src_offset))
            return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: example %d reads %llu bytes at %lld, outside the %zu-byte source", who, n, need,
                                   d.src_offset, src_bytes);
        out.d[n] = d;
    }
    return 0;
}

// The same for crop descriptors: the virtual oh x ow may exceed the canvas, the window may not, and it lies inside the virtual resize.
template <class Bytes>
int check_crop(const char *who, const unsigned char *src, size_t src_bytes, const mrcnn_crop_desc_t *desc, int N, const void *dst,
               int dst_h, int dst_w, int G, Bytes elem_bytes, Descs<mrcnn_crop_desc_t> &out) {
    if (!desc || !dst) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null pointer", who);
    if (N < 1 || N > MRCNN_RESIZE_BATCH_MAX)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: N = %d outside 1..%d", who, N, MRCNN_RESIZE_BATCH_MAX);
    if (dst_h <= 0 || dst_w <= 0 || (long long)dst_h * ((long long)dst_w + 15) > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad output size %d x %d", who, dst_h, dst_w);
    if (reinterpret_cast<uintptr_t>(dst) & 15) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: dst not 16-byte aligned", who);
    for (int n = 0; n < N; ++n) {
        const mrcnn_crop_desc_t &d = desc[n];
        if (d.H <= 0 || d.W <= 0 || d.oh <= 0 || d.ow <= 0 || (d.flip != 0 && d.flip != 1) || d.count < 0 || d.count > G || d.src_offset < 0)
            return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad descriptor %d (H %d W %d oh %d ow %d flip %d count %d offset %lld)", who, n,
                                   d.H, d.W, d.oh, d.ow, d.flip, d.count, d.src_offset);
        if (d.y0 < 0 || d.x0 < 0 || d.ch <= 0 || d.cw <= 0 || d.ch > dst_h || d.cw > dst_w || d.ch > d.oh - d.y0 || d.cw > d.ow - d.x0)
            return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: bad window in descriptor %d (y0 %d x0 %d ch %d cw %d of %d x %d, canvas %d x %d)",
                                   who, n, d.y0, d.x0, d.ch, d.cw, d.oh, d.ow, dst_h, dst_w);
        const unsigned long long need = elem_bytes(d);
        if (need > 0 && (!src || (unsigned long long)d.src_offset > src_bytes || need > src_bytes - (unsigned long long)d.src_offset))
            return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: example %d reads %llu bytes at %lld, outside the %zu-byte source", who, n, need,
                                   d.src_offset, src_bytes);
        out.d[n] = d;
    }
    return 0;
}

}  // namespace

extern "C" int mrcnn_image_resize_batch_u8_f32(const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, float *dst,
                                               int dst_h, int dst_w, float div, void *stream) {
    Descs<mrcnn_resize_desc_t> ds = {};
    if (int e = check_batch("image_resize_batch", src, src_bytes, desc, N, dst, dst_h, dst_w, 0, [](const mrcnn_resize_desc_t &d) {
            return (unsigned long long)d.H * d.W * 3; }, ds))
        return e;
    const int wq = (dst_w + 3) / 4;
    hipLaunchKernelGGL(k_image_resize_batch_u8<mrcnn_resize_desc_t>, dim3(mrcnn::cdiv((long long)dst_h * wq, NT), N), dim3(NT), 0, (hipStream_t)stream, src, ds,
                       dst, dst_h, dst_w, wq, div);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_mask_resize_batch_nearest_u8(const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, int G,
                                                  unsigned char *dst, int dst_h, int dst_w, void *stream) {
    if (G < 1 || G > 65535) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_resize_batch: G = %d outside 1..65535", G);
    Descs<mrcnn_resize_desc_t> ds = {};
    if (int e = check_batch("mask_resize_batch", src, src_bytes, desc, N, dst, dst_h, dst_w, G, [](const mrcnn_resize_desc_t &d) {
            return (unsigned long long)d.count * d.H * d.W; }, ds))
        return e;
    const int wq = (dst_w + 15) / 16;
    hipLaunchKernelGGL(k_mask_resize_batch_u8<mrcnn_resize_desc_t>, dim3(mrcnn::cdiv((long long)dst_h * wq, NT), G, N), dim3(NT), 0,
                       (hipStream_t)stream, src, ds, (const int32_t *)nullptr, dst, G, dst_h, dst_w, wq);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_image_resize_crop_batch_u8_f32(const unsigned char *src, size_t src_bytes, const mrcnn_crop_desc_t *desc, int N,
                                                    float *dst, int dst_h, int dst_w, float div, void *stream) {
    Descs<mrcnn_crop_desc_t> ds = {};
    if (int e = check_crop("image_resize_crop_batch", src, src_bytes, desc, N, dst, dst_h, dst_w, 0, [](const mrcnn_crop_desc_t &d) {
            return (unsigned long long)d.H * d.W * 3; }, ds))
        return e;
    const int wq = (dst_w + 3) / 4;
    hipLaunchKernelGGL(k_image_resize_batch_u8<mrcnn_crop_desc_t>, dim3(mrcnn::cdiv((long long)dst_h * wq, NT), N), dim3(NT), 0,
                       (hipStream_t)stream, src, ds, dst, dst_h, dst_w, wq, div);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_mask_crop_boxes_u8(const unsigned char *src, size_t src_bytes, const mrcnn_crop_desc_t *desc, int N, int Gin, int G,
                                        int dst_h, int dst_w, const int32_t *labels_in, float *bboxes, int32_t *labels, int32_t *gather,
                                        int32_t *ws, void *stream) {
    if (Gin < 1 || Gin > 65535 || G < 1 || G > 65535)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_crop_boxes: Gin = %d / G = %d outside 1..65535", Gin, G);
    if (!labels_in || !labels || !gather || !ws) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_crop_boxes: null pointer");
    if (reinterpret_cast<uintptr_t>(ws) & 15) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_crop_boxes: ws not 16-byte aligned");
    Descs<mrcnn_crop_desc_t> ds = {};
    if (int e = check_crop("mask_crop_boxes", src, src_bytes, desc, N, bboxes, dst_h, dst_w, Gin, [](const mrcnn_crop_desc_t &d) {
            return (unsigned long long)d.count * d.H * d.W; }, ds))
        return e;
    MRCNN_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)N * Gin * 4 * sizeof(int32_t), (hipStream_t)stream));
    const int wq = (dst_w + 15) / 16;
    hipLaunchKernelGGL(k_mask_crop_reduce, dim3(mrcnn::cdiv((long long)dst_h * wq, NT), Gin, N), dim3(NT), 0, (hipStream_t)stream, src, ds,
                       ws, Gin, dst_h, dst_w, wq);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mask_crop_finalize, dim3(N), dim3(kWave), 0, (hipStream_t)stream, ds, ws, labels_in, bboxes, labels, gather, Gin,
                       G, dst_h, dst_w);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_mask_resize_crop_batch_nearest_u8(const unsigned char *src, size_t src_bytes, const mrcnn_crop_desc_t *desc, int N,
                                                       int G, const int32_t *gather, unsigned char *dst, int dst_h, int dst_w,
                                                       void *stream) {
    if (G < 1 || G > 65535) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_resize_crop_batch: G = %d outside 1..65535", G);
    if (!gather) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_resize_crop_batch: null gather table");
    Descs<mrcnn_crop_desc_t> ds = {};
    if (int e = check_crop("mask_resize_crop_batch", src, src_bytes, desc, N, dst, dst_h, dst_w, 65535, [](const mrcnn_crop_desc_t &d) {
            return (unsigned long long)d.count * d.H * d.W; }, ds))
        return e;
    const int wq = (dst_w + 15) / 16;
    hipLaunchKernelGGL(k_mask_resize_batch_u8<mrcnn_crop_desc_t>, dim3(mrcnn::cdiv((long long)dst_h * wq, NT), G, N), dim3(NT), 0,
                       (hipStream_t)stream, src, ds, gather, dst, G, dst_h, dst_w, wq);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
