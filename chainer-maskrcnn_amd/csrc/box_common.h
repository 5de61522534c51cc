// The box arithmetic, stated once and shared by the proposal path of rpn.hip, the samplers of targets.hip, the
// stage-to-stage step of cascade.hip, the IoU losses of box_loss.hip and, through detect_common.h, the inference post-processing of
// predict.hip, tta.hip and boxpost.hip: a refined box is decoded, clipped, matched, levelled and encoded with the bits every other
// kernel gives it.  Float arithmetic follows oracle/boxes.py operation for operation: no contraction, correctly rounded division; the
// parenthesisation is the rounding order.  Boxes are (y1, x1, y2, x2), locs (dy, dx, dh, dw), a centre / size (cy, cx, h, w).
//   loc_denorm4, loc_norm4           v * std + mean; (loc - mean) / std
//   box_cs, loc2cs, cs_corners       ChainerCV loc2bbox in its steps (utils/proposal_creator.py; maskrcnn.py:196); loc2bbox is the three
//   box_clip                         the clip to the image                  (maskrcnn.py:202-203)
//   match_iou, max_arg_step          ChainerCV bbox_iou, iou.max / argmax   (utils/proposal_target_creator.py:55-57)
//   nms_inter, nms_union, nms_iou, nms_suppresses   ChainerCV non_maximum_suppression's IoU: sides clamped at 0, the area of b passed in
//   bbox2loc                         ChainerCV bbox2loc                     (utils/proposal_target_creator.py:88)
//   fpn_level                        map_rois_to_fpn_levels                 (model/rpn/multilevel_region_proposal_network.py:16-31)
// The forms (float4 by value, loc_norm4 in place, two scalar NMS terms, not a pair) are the ones that keep the callers' machine code.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

constexpr float kEps = 1.1920929e-07f;   // np.finfo(np.float32).eps

__device__ __forceinline__ float4 loc_denorm4(float4 v, float4 stdv, float4 mean) {
    return make_float4(v.x * stdv.x + mean.x, v.y * stdv.y + mean.y, v.z * stdv.z + mean.z, v.w * stdv.w + mean.w);
}
__device__ __forceinline__ void loc_norm4(float4 &loc, const float4 &mean, const float4 &stdv) {      // in place
    loc.x = (loc.x - mean.x) / stdv.x; loc.y = (loc.y - mean.y) / stdv.y;
    loc.z = (loc.z - mean.z) / stdv.z; loc.w = (loc.w - mean.w) / stdv.w;
}

// loc2bbox: the centre / size of box b; the centre / size of the box that loc d decodes to against a source of centre / size s (dh, dw
// are not clamped here; the scalar rules are box_loss.hip's too, which clamps first); the corners of a centre / size.
__device__ __forceinline__ float4 box_cs(float4 b) {
    const float h = b.z - b.x, w = b.w - b.y;
    return make_float4(b.x + 0.5f * h, b.y + 0.5f * w, h, w);
}
__device__ __forceinline__ float loc2centre1(float d, float size, float centre) { return d * size + centre; }
__device__ __forceinline__ float loc2size1(float d, float size) { return expf(d) * size; }
__device__ __forceinline__ float4 loc2cs(float4 s, float4 d) {
    return make_float4(loc2centre1(d.x, s.z, s.x), loc2centre1(d.y, s.w, s.y), loc2size1(d.z, s.z), loc2size1(d.w, s.w));
}
__device__ __forceinline__ float4 cs_corners(float4 cs) {
    return make_float4(cs.x - 0.5f * cs.z, cs.y - 0.5f * cs.w, cs.x + 0.5f * cs.z, cs.y + 0.5f * cs.w);
}
__device__ __forceinline__ float4 loc2bbox(float4 src, float4 d) { return cs_corners(loc2cs(box_cs(src), d)); }

// Every corner into [0, lim]; fminf / fmaxf drop a NaN, so the clipped box is finite whatever the deltas were.
__device__ __forceinline__ float clip1(float v, float lim) { return fmaxf(fminf(v, lim), 0.f); }
__device__ __forceinline__ float4 box_clip(float4 b, float lim_h, float lim_w) {
    const float y1 = clip1(b.x, lim_h), y2 = clip1(b.z, lim_h), x1 = clip1(b.y, lim_w), x2 = clip1(b.w, lim_w);
    return make_float4(y1, x1, y2, x2);
}

__device__ __forceinline__ float match_iou(const float4 a, const float4 b) {
    // ChainerCV bbox_iou: area_i = prod(br - tl) * all(tl < br); iou = area_i / (area_a + area_b - area_i)
    const float tly = fmaxf(a.x, b.x), tlx = fmaxf(a.y, b.y);
    const float bry = fminf(a.z, b.z), brx = fminf(a.w, b.w);
    float area_i = (bry - tly) * (brx - tlx);
    area_i = area_i * ((tly < bry && tlx < brx) ? 1.0f : 0.0f);
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    return area_i / ((area_a + area_b) - area_i);
}

// One step of iou.max(axis=1) / argmax of NumPy over a row of ground-truth boxes, g ascending from 0 with v = match_iou(b, box g): the
// first maximum; a NaN (0 / 0: two zero-area boxes) wins over every number and the first NaN stays.
__device__ __forceinline__ void max_arg_step(int g, float v, float &best, int &arg) {
    const float cur = best;
    if (g == 0 || v > cur || (v != v && cur == cur)) { best = v; arg = g; }
}

// Box b (of area area_b, the product of its sides) against box c, ChainerCV's non_maximum_suppression: the intersection ai with its
// sides clamped at 0 and the union u = (area_b + area_c) - ai; the IoU ai / u as a value, the division correctly rounded (two zero-area
// boxes give NaN; the callers' comparisons are written so that NaN has no effect); b suppresses c where IoU >= thresh.
__device__ __forceinline__ float nms_inter(float4 b, float4 c) {
    const float top = fmaxf(b.x, c.x), left = fmaxf(b.y, c.y), bottom = fminf(b.z, c.z), right = fminf(b.w, c.w);
    const float hgt = fmaxf(bottom - top, 0.f), wid = fmaxf(right - left, 0.f);
    return hgt * wid;
}
__device__ __forceinline__ float nms_union(float area_b, float4 c, float ai) { return (area_b + (c.z - c.x) * (c.w - c.y)) - ai; }
__device__ __forceinline__ float nms_iou(float4 b, float area_b, float4 c) {
    const float ai = nms_inter(b, c);
    return ai / nms_union(area_b, c, ai);
}
__device__ __forceinline__ bool nms_suppresses(float4 b, float area_b, float4 c, float thresh) { return nms_iou(b, area_b, c) >= thresh; }

__device__ __forceinline__ float4 bbox2loc(const float4 s, const float4 d) {
    float h = s.z - s.x, w = s.w - s.y;
    const float cy = s.x + 0.5f * h, cx = s.y + 0.5f * w;
    const float bh = d.z - d.x, bw = d.w - d.y;
    const float bcy = d.x + 0.5f * bh, bcx = d.y + 0.5f * bw;
    h = fmaxf(h, kEps);
    w = fmaxf(w, kEps);
    return make_float4((bcy - cy) / h, (bcx - cx) / w, logf(bh / h), logf(bw / w));
}

// floor(4 + log2(sqrt(area) / 224 + 1e-6)) clipped to [k_min, k_max]; the samplers pass 0, 4.
__device__ __forceinline__ float fpn_level(float4 b, float k_min, float k_max) {
    const float area = (b.z - b.x) * (b.w - b.y);
    const float v = sqrtf(area) / 224.0f + 1e-6f;
    const float t = floorf(4.0f + (float)log2((double)v));
    return fminf(fmaxf(t, k_min), k_max);
}
