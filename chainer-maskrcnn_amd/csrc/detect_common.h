// The arithmetic of the inference post-processing, stated once and shared by the single-view kernels of predict.hip
// and the multi-view kernels of tta.hip, so one unmirrored view gives predict()'s bits by construction; rpn.hip takes orderable().
// Float arithmetic follows oracle/predict.py operation for operation: no contraction, correctly rounded division.
//   decode       chainer_maskrcnn/model/maskrcnn.py:178-205  (un-scale, loc2bbox, clip, softmax)
//   candidates   maskrcnn.py:278-312  (_suppress: prob > score_thresh, score descending then index descending, ChainerCV NMS)
//   paste        maskrcnn.py:231-246  (cv2.resize to the box, *255, truncate, > 127, paste)
// and the score weight of Soft-NMS and box voting (boxpost.hip).  The box arithmetic inside them (de-normalised loc,
// loc2bbox, clip, nms_iou / nms_suppresses) is box_common.h's, the functions the training kernels call.
#pragma once
#include <hip/hip_runtime.h>
#include "box_common.h"

#pragma clang fp contract(off)

typedef unsigned long long u64;

constexpr int CN_CAP = 512;         // most RoIs of the all-in-LDS class NMS (k_class_nms); above it mrcnn_class_nms_ws_f32's workspace kernels

__device__ __forceinline__ unsigned orderable(float f) {     // monotone float -> uint
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The softmax of one box_out row's n_class scores (F.softmax, maskrcnn.py:205): the maximum, the sum of expf(o[c] - m) in class order, and
// class c's probability expf(o[c] - m) / s.  Shared by detect_decode_row and the stage mean of cascade.hip.
struct SoftmaxStats { float m, s; };

__device__ __forceinline__ SoftmaxStats detect_softmax_stats(const float *__restrict__ o, int n_class) {
    float m = -INFINITY;
    for (int c = 0; c < n_class; ++c) m = fmaxf(m, o[c]);
    float s = 0.f;
    for (int c = 0; c < n_class; ++c) s += expf(o[c] - m);
    return SoftmaxStats{m, s};
}

__device__ __forceinline__ float detect_softmax_prob(float v, SoftmaxStats st) { return expf(v - st.m) / st.s; }

// One RoI (y1,x1,y2,x2) of the forward's scaled image and its box_out row o (n_class scores, then the class-agnostic loc at loc0):
// the box in original-image pixels, clipped to size; softmax over the n_class scores into prob_row.
__device__ __forceinline__ float4 detect_decode_row(const float *__restrict__ roi, const float *__restrict__ o, int n_class, int loc0,
                                                    float scale, float4 mean, float4 stdv, float size_h, float size_w,
                                                    float *__restrict__ prob_row) {
    const float4 rr = *reinterpret_cast<const float4 *>(roi);
    const float4 r = make_float4(rr.x / scale, rr.y / scale, rr.z / scale, rr.w / scale);         // roi = rois / scale (:178)
    const float4 d = loc_denorm4(make_float4(o[loc0], o[loc0 + 1], o[loc0 + 2], o[loc0 + 3]), stdv, mean);   // (:191-195)
    const float4 b = box_clip(loc2bbox(r, d), size_h, size_w);                                     // loc2bbox (:196), clip (:202-203)
    const SoftmaxStats st = detect_softmax_stats(o, n_class);
    for (int c = 0; c < n_class; ++c) prob_row[c] = detect_softmax_prob(o[c], st);                 // F.softmax (:205)
    return b;
}

// NMS candidate i with class probability p: valid | orderable score << 31 | index, 0 when p <= score_thresh.  Descending key order is
// (score descending, index descending), the oracle's pin of argsort()[::-1]; the zero keys come last.
__device__ __forceinline__ u64 candidate_key(float p, float score_thresh, int i) {
    return p > score_thresh ? (1ull << 63) | ((u64)orderable(p) << 31) | (u64)i : 0ull;
}
__device__ __forceinline__ int candidate_index(u64 key) { return (int)(key & 0x7FFFFFFFull); }

// Bitonic sort, descending, of skey[0..P) in LDS (P a power of two) by a workgroup of T threads.  The keys are visible to the workgroup
// on entry (a barrier after they were written) and the sorted keys are on return.
template <int T>
__device__ __forceinline__ void bitonic_sort_desc(u64 *skey, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const u64 a = skey[i], b = skey[ixj];
                    const bool up = (i & k) == 0;
                    if ((a < b) == up) { skey[i] = b; skey[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// The weight a selected box puts on the score of a remaining candidate of its class at this IoU (Soft-NMS, Bodla et al. 2017; method =
// SOFT_NMS_*, the values of the public header's MRCNN_SOFT_NMS_*): hard 0 at iou >= nms_thresh; linear 1 - iou at iou >= nms_thresh; gaussian expf(-(iou * iou) / sigma) at iou > 0;
// 1 otherwise (a NaN IoU included).
enum { SOFT_NMS_HARD = 0, SOFT_NMS_LINEAR = 1, SOFT_NMS_GAUSSIAN = 2 };

__device__ __forceinline__ float soft_nms_weight(int method, float iou, float nms_thresh, float sigma) {
    if (method == SOFT_NMS_GAUSSIAN) return iou > 0.f ? expf(-(iou * iou) / sigma) : 1.0f;
    if (iou >= nms_thresh) return method == SOFT_NMS_LINEAR ? 1.0f - iou : 0.0f;
    return 1.0f;
}

// Mask paste of one detection (maskrcnn.py:231-246): the S x S map m(yy, xx) = tap(yy, xx) goes through cv2.resize(m, (w, h)), float
// bilinear (half-pixel centres, edge clamp); *255 -> uint8 (truncate) -> > 127; pasted at (int(y1), int(x1)) of box b, clipped to the
// H x W image o.  Grid-stride over the pixels along blockIdx.x with 256-thread workgroups.
template <class Tap>
__device__ __forceinline__ void mask_paste_box(float4 b, int S, int H, int W, unsigned char *__restrict__ o, Tap tap) {
    const int mw = (int)(b.w - b.y), mh = (int)(b.z - b.x);
    const int s0 = (int)b.x, t0 = (int)b.y;
    const double sy = mh > 0 ? 1.0 / ((double)mh / (double)S) : 0.0, sx = mw > 0 ? 1.0 / ((double)mw / (double)S) : 0.0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < H * W; p += gridDim.x * 256) {
        const int y = p / W, x = p % W;
        const int dy = y - s0, dx = x - t0;
        unsigned char v = 0;
        if (dy >= 0 && dy < mh && dx >= 0 && dx < mw) {
            float fy = (float)(((double)dy + 0.5) * sy - 0.5), fx = (float)(((double)dx + 0.5) * sx - 0.5);
            int iy = (int)floorf(fy), ix = (int)floorf(fx);
            fy -= (float)iy; fx -= (float)ix;
            if (iy < 0) { fy = 0.f; iy = 0; }
            if (iy >= S - 1) { fy = 0.f; iy = S - 1; }
            if (ix < 0) { fx = 0.f; ix = 0; }
            if (ix >= S - 1) { fx = 0.f; ix = S - 1; }
            const int iy1 = min(iy + 1, S - 1), ix1 = min(ix + 1, S - 1);
            const float r0 = tap(iy, ix) * (1.0f - fx) + tap(iy, ix1) * fx;
            const float r1 = tap(iy1, ix) * (1.0f - fx) + tap(iy1, ix1) * fx;
            const float m = r0 * (1.0f - fy) + r1 * fy;
            const int q = (int)(m * 255.0f);
            v = (unsigned char)((q & 0xFF) > 127 ? 1 : 0);
        }
        o[p] = v;
    }
}
