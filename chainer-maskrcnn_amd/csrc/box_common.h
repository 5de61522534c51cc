// The box arithmetic of the training targets, stated once and shared by the samplers of targets.hip and the stage-to-stage step of
// cascade.hip, so a refined box is matched, levelled and encoded with the bits the sampler gives a proposal.
// Float arithmetic follows oracle/boxes.py operation for operation: no contraction, correctly rounded division.
//   box_iou     ChainerCV bbox_iou            (utils/proposal_target_creator.py:55)
//   bbox2loc    ChainerCV bbox2loc            (utils/proposal_target_creator.py:88)
//   fpn_level   map_rois_to_fpn_levels        (model/rpn/multilevel_region_proposal_network.py:16-31)
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

constexpr float kEps = 1.1920929e-07f;   // np.finfo(np.float32).eps

__device__ __forceinline__ float box_iou(const float4 a, const float4 b) {
    // ChainerCV bbox_iou: area_i = prod(br - tl) * all(tl < br); iou = area_i / (area_a + area_b - area_i)
    const float tly = fmaxf(a.x, b.x), tlx = fmaxf(a.y, b.y);
    const float bry = fminf(a.z, b.z), brx = fminf(a.w, b.w);
    float area_i = (bry - tly) * (brx - tlx);
    area_i = area_i * ((tly < bry && tlx < brx) ? 1.0f : 0.0f);
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    return area_i / ((area_a + area_b) - area_i);
}

__device__ __forceinline__ float4 bbox2loc(const float4 s, const float4 d) {
    float h = s.z - s.x, w = s.w - s.y;
    const float cy = s.x + 0.5f * h, cx = s.y + 0.5f * w;
    const float bh = d.z - d.x, bw = d.w - d.y;
    const float bcy = d.x + 0.5f * bh, bcx = d.y + 0.5f * bw;
    h = fmaxf(h, kEps);
    w = fmaxf(w, kEps);
    return make_float4((bcy - cy) / h, (bcx - cx) / w, logf(bh / h), logf(bw / w));
}

__device__ __forceinline__ float fpn_level(float4 b) {
    const float area = (b.z - b.x) * (b.w - b.y);
    const float v = sqrtf(area) / 224.0f + 1e-6f;
    const float t = floorf(4.0f + (float)log2((double)v));
    return fminf(fmaxf(t, 0.f), 4.f);
}
