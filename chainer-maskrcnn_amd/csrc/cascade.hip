// Cascade R-CNN box stages (Cai & Vasconcelos 2018; Detectron2's CascadeROIHeads) on the device for gfx950: the step between two box
// stages and the inference score.  No counterpart in the reference, whose RoI head has one stage.
//   mrcnn_cascade_refine_f32  stage k's input boxes + its box_out -> stage k+1's input boxes, levels, labels and targets, one launch
//   mrcnn_cascade_prob_f32    the K stages' box_out -> the mean of their softmax scores, one launch
// Both are latency-bound: R = N * S is a few thousand rows, G tens of boxes (bytes in DESIGN.md section 3.21).
//
// The rules of cascade_refine, row r of image i (float32, operation for operation, FP contraction off; restated in NumPy by
// tests/cascade_reference.py):
//   padding   prev_label[r] < 0: roi = 0, xy5 = (i,0,0,0,0), level 0, gt_loc = 0, label -1, assign -1.
//   decode    box_clip(loc2bbox(rois[r], loc_denorm4(o[loc0 ..], std_prev, mean)), h, w) of box_common.h with image i's h / w: what
//             detect_decode_row calls after its un-scale.  dh / dw are not clamped: an expf that overflows gives -inf / +inf corners,
//             which clip to the full extent; fminf / fmaxf drop a NaN, so the box is finite whatever the deltas are.
//   level     fpn_level(b, 0, 4) (box_common.h) of the refined box: the sampler's level of a ground-truth box.
//   xy5       (i, x1, y1, x2, y2) of the refined box.
//   -- with ground truth only --
//   empty     y2 - y1 <= 0 or x2 - x1 <= 0 after clipping: label -1 (both losses ignore the row; the fixed-shape form of Detectron2
//             dropping empty boxes between stages), assign -1, gt_loc = 0.  The box and the level are written as computed.
//   no gt     G = min(n_gt[i], gt_cap) == 0: label 0, assign -1, gt_loc = 0.
//   match     match_iou (box_common.h) against the image's first G boxes; max / argmax by max_arg_step, as k_proposal_target: NumPy's,
//             the first maximum, a NaN wins and the first NaN stays.  label = gt_labels[arg] + 1 where max >= iou_thresh (false for a NaN
//             maximum), else 0; assign = arg.
//   targets   label > 0: gt_loc = bbox2loc(roi, gt[arg]) through loc_norm4(mean, std_next); every other row zeros, so no -inf of a
//             zero-size box reaches a loss.
// One thread per row; the image's ground-truth boxes are staged in LDS, so a workgroup never straddles two images:
// grid (ceil(S / 256), N).
#include "common.h"
#include "box_common.h"
#include "detect_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_GCAP = 256;       // most ground-truth boxes per image (4 KiB of LDS)

__global__ __launch_bounds__(CR_THREADS) void k_cascade_refine(
    const float *__restrict__ rois, const float *__restrict__ box_out, int ld, int loc0, const int32_t *__restrict__ prev_label, int S,
    float4 mean, float4 std_prev, const float *__restrict__ per_image_hw, float img_h, float img_w,
    const float *__restrict__ gt_boxes, const int32_t *__restrict__ gt_labels, const int32_t *__restrict__ n_gt, int gt_cap,
    float iou_thresh, float4 std_next, float *__restrict__ roi_out, float *__restrict__ rois_xy5, int32_t *__restrict__ levels,
    float *__restrict__ gt_loc, int32_t *__restrict__ label, int32_t *__restrict__ gt_assign) {
    __shared__ float4 sg[CR_GCAP];
    const int img = blockIdx.y;
    const bool train = gt_boxes != nullptr;
    const int G = train ? max(min(min(n_gt[img], gt_cap), CR_GCAP), 0) : 0;
    for (int g = threadIdx.x; g < G; g += CR_THREADS) sg[g] = *reinterpret_cast<const float4 *>(gt_boxes + ((size_t)img * gt_cap + g) * 4);
    __syncthreads();
    const int j = blockIdx.x * CR_THREADS + threadIdx.x;
    if (j >= S) return;
    const size_t row = (size_t)img * S + j;
    if (per_image_hw) { img_h = per_image_hw[2 * img]; img_w = per_image_hw[2 * img + 1]; }
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f), loc = make_float4(0.f, 0.f, 0.f, 0.f);
    int lev = 0, lab = -1, arg = -1;
    if (!prev_label || prev_label[row] >= 0) {
        const float4 r = *reinterpret_cast<const float4 *>(rois + row * 4);
        const float *o = box_out + row * ld;
        const float4 d = loc_denorm4(make_float4(o[loc0], o[loc0 + 1], o[loc0 + 2], o[loc0 + 3]), std_prev, mean);
        b = box_clip(loc2bbox(r, d), img_h, img_w);
        lev = (int)fpn_level(b, 0.f, 4.f);
        if (train && !(b.z - b.x <= 0.f || b.w - b.y <= 0.f)) {
            lab = 0;
            if (G > 0) {
                float best = -INFINITY;
                arg = 0;
                for (int g = 0; g < G; ++g) max_arg_step(g, match_iou(b, sg[g]), best, arg);
                if (best >= iou_thresh) {
                    lab = gt_labels[(size_t)img * gt_cap + arg] + 1;
                    if (lab > 0) { loc = bbox2loc(b, sg[arg]); loc_norm4(loc, mean, std_next); }
                }
            }
        }
    }
    *reinterpret_cast<float4 *>(roi_out + row * 4) = b;
    float *r5 = rois_xy5 + row * 5;
    r5[0] = (float)img; r5[1] = b.y; r5[2] = b.x; r5[3] = b.w; r5[4] = b.z;
    levels[row] = lev;
    if (train) {
        *reinterpret_cast<float4 *>(gt_loc + row * 4) = loc;
        label[row] = lab;
        gt_assign[row] = arg;
    }
}

constexpr int CP_MAXK = 4;
struct StagePtrs { const float *o[CP_MAXK]; };

// One wave per row: every lane takes the K softmax statistics of the row (the sequential sums of detect_decode_row; the loads are
// broadcasts), then lane l writes the classes l, l + 64, ...: the stages' probabilities added in stage order, divided by (float)K.
__global__ __launch_bounds__(64) void k_cascade_prob(StagePtrs sp, int K, int ld, int n_class, float *__restrict__ prob) {
    const size_t row = blockIdx.x;
    SoftmaxStats st[CP_MAXK];
#pragma unroll
    for (int k = 0; k < CP_MAXK; ++k)
        if (k < K) st[k] = detect_softmax_stats(sp.o[k] + row * ld, n_class);
    for (int c = threadIdx.x; c < n_class; c += 64) {
        float p = detect_softmax_prob(sp.o[0][row * ld + c], st[0]);
#pragma unroll
        for (int k = 1; k < CP_MAXK; ++k)
            if (k < K) p = p + detect_softmax_prob(sp.o[k][row * ld + c], st[k]);
        prob[row * n_class + c] = p / (float)K;
    }
}

}  // namespace

extern "C" int mrcnn_cascade_refine_f32(const float *rois, const float *box_out, int ld, int loc0, const int32_t *prev_label, int N,
                                        int S, const float *loc_mean4, const float *std_prev4, const float *per_image_hw, float img_h,
                                        float img_w, const float *gt_boxes, const int32_t *gt_labels, const int32_t *n_gt, int gt_cap,
                                        float iou_thresh, const float *std_next4, float *roi, float *rois_xy5, int32_t *levels,
                                        float *gt_loc, int32_t *label, int32_t *gt_assign, void *stream) {
    if (N < 0 || S < 0 || N > 65535) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_refine: bad sizes (0 <= N <= 65535, S >= 0)");
    if (!loc_mean4 || !std_prev4) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_refine: null mean / std");
    if (N == 0 || S == 0) return 0;
    if (!rois || !box_out || !roi || !rois_xy5 || !levels) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_refine: null pointer");
    if (loc0 < 0 || ld < loc0 + 4) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_refine: ld %d < loc0 %d + 4", ld, loc0);
    const bool train = gt_boxes != nullptr;
    if (train) {
        if (!gt_labels || !n_gt || !std_next4 || !gt_loc || !label || !gt_assign)
            return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_refine: ground truth without its labels, counts, std or outputs");
        if (gt_cap <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_refine: gt_cap %d", gt_cap);
        if (gt_cap > CR_GCAP) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "cascade_refine: %d gt boxes per image > %d", gt_cap, CR_GCAP);
    } else if (gt_labels || n_gt || gt_loc || label || gt_assign) {
        return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_refine: ground-truth arguments without gt_boxes");
    }
    const float4 mean = make_float4(loc_mean4[0], loc_mean4[1], loc_mean4[2], loc_mean4[3]);
    const float4 sp = make_float4(std_prev4[0], std_prev4[1], std_prev4[2], std_prev4[3]);
    const float4 sn = train ? make_float4(std_next4[0], std_next4[1], std_next4[2], std_next4[3]) : make_float4(1.f, 1.f, 1.f, 1.f);
    hipLaunchKernelGGL(k_cascade_refine, dim3(mrcnn::cdiv(S, CR_THREADS), N), dim3(CR_THREADS), 0, (hipStream_t)stream, rois, box_out, ld,
                       loc0, prev_label, S, mean, sp, per_image_hw, img_h, img_w, gt_boxes, gt_labels, n_gt, gt_cap, iou_thresh, sn, roi,
                       rois_xy5, levels, gt_loc, label, gt_assign);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_cascade_prob_f32(const float *box_out0, const float *box_out1, const float *box_out2, const float *box_out3, int K,
                                      int R, int ld, int n_class, float *prob, void *stream) {
    if (K < 2 || K > CP_MAXK) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_prob: %d stages (2 .. %d)", K, CP_MAXK);
    if (R < 0 || n_class <= 0 || ld < n_class) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_prob: bad sizes");
    if (R == 0) return 0;
    StagePtrs sp{{box_out0, box_out1, box_out2, box_out3}};
    for (int k = 0; k < K; ++k)
        if (!sp.o[k]) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_prob: stage %d of %d is NULL", k + 1, K);
    if (!prob) return mrcnn::fail_arg(MRCNN_E_INVALID, "cascade_prob: null output");
    hipLaunchKernelGGL(k_cascade_prob, dim3(R), dim3(64), 0, (hipStream_t)stream, sp, K, ld, n_class, prob);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
