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
#include "common.h"
#include "resize_common.h"

namespace {

constexpr int NT = 256;

struct Descs {
    mrcnn_resize_desc_t d[MRCNN_RESIZE_BATCH_MAX];
};

// grid (cdiv(dst_h * wq, NT), N); wq = cdiv(dst_w, 4)
__global__ __launch_bounds__(NT) void k_image_resize_batch_u8(const uint8_t *__restrict__ src, const Descs ds, float *__restrict__ dst,
                                                              int dst_h, int dst_w, int wq, float div) {
    const int n = blockIdx.y;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= dst_h * wq) return;
    const mrcnn_resize_desc_t d = ds.d[n];
    const int y = i / wq, x0 = (i - y * wq) * 4;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[c][j] = 0.f;
    if (y < d.oh) {
        int y0, y1;
        float b0, b1;
        linear_tap(y, d.oh, d.H, y0, y1, b0, b1);
        const uint8_t *base = src + d.src_offset;
        const uint8_t *r0 = base + (size_t)y0 * d.W * 3, *r1 = base + (size_t)y1 * d.W * 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x < d.ow) {
                int s0, s1;
                float a0, a1;
                linear_tap(x, d.ow, d.W, s0, s1, a0, a1);
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

// grid (cdiv(dst_h * wq, NT), G, N); wq = cdiv(dst_w, 16)
__global__ __launch_bounds__(NT) void k_mask_resize_batch_u8(const uint8_t *__restrict__ src, const Descs ds, uint8_t *__restrict__ dst,
                                                             int G, int dst_h, int dst_w, int wq) {
    const int n = blockIdx.z, g = blockIdx.y;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= dst_h * wq) return;
    const mrcnn_resize_desc_t d = ds.d[n];
    const int y = i / wq, x0 = (i - y * wq) * 16;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (g < d.count && y < d.oh) {
        const int sy = nearest_tap(y, d.oh, d.H);
        const uint8_t *row = src + d.src_offset + ((size_t)g * d.H + sy) * d.W;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int x = x0 + j;
            if (x < d.ow) {
                int sx = nearest_tap(x, d.ow, d.W);
                if (d.flip) sx = d.W - 1 - sx;
                w[j >> 2] |= (unsigned)row[sx] << (8 * (j & 3));
            }
        }
    }
    uint8_t *o = dst + (((size_t)n * G + g) * dst_h + y) * dst_w + x0;
    if ((dst_w & 15) == 0) {
        *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (x0 + j < dst_w) o[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

// Common argument checks; elem_bytes(d) = the source bytes example d reads.  Returns 0 or an MRCNN_E_* code (error already set).
template <class Bytes>
int check_batch(const char *who, const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, const void *dst,
                int dst_h, int dst_w, int G, Bytes elem_bytes, Descs &out) {
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

}  // namespace

extern "C" int mrcnn_image_resize_batch_u8_f32(const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, float *dst,
                                               int dst_h, int dst_w, float div, void *stream) {
    Descs ds = {};
    if (int e = check_batch("image_resize_batch", src, src_bytes, desc, N, dst, dst_h, dst_w, 0, [](const mrcnn_resize_desc_t &d) {
            return (unsigned long long)d.H * d.W * 3; }, ds))
        return e;
    const int wq = (dst_w + 3) / 4;
    hipLaunchKernelGGL(k_image_resize_batch_u8, dim3(mrcnn::cdiv((long long)dst_h * wq, NT), N), dim3(NT), 0, (hipStream_t)stream, src, ds,
                       dst, dst_h, dst_w, wq, div);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_mask_resize_batch_nearest_u8(const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, int G,
                                                  unsigned char *dst, int dst_h, int dst_w, void *stream) {
    if (G < 1 || G > 65535) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_resize_batch: G = %d outside 1..65535", G);
    Descs ds = {};
    if (int e = check_batch("mask_resize_batch", src, src_bytes, desc, N, dst, dst_h, dst_w, G, [](const mrcnn_resize_desc_t &d) {
            return (unsigned long long)d.count * d.H * d.W; }, ds))
        return e;
    const int wq = (dst_w + 15) / 16;
    hipLaunchKernelGGL(k_mask_resize_batch_u8, dim3(mrcnn::cdiv((long long)dst_h * wq, NT), G, N), dim3(NT), 0, (hipStream_t)stream, src,
                       ds, dst, G, dst_h, dst_w, wq);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
