// Inference post-processing on the device for gfx950: box decode + softmax, per-class
// score filter + NMS, mask paste.  Replaces the host NumPy / OpenCV code of
//   chainer_maskrcnn/model/maskrcnn.py:178-210  (un-scale, loc2bbox, clip, softmax, D2H)
//   chainer_maskrcnn/model/maskrcnn.py:278-312  (_suppress: per class, prob > score_thresh, ChainerCV NMS 0.3)
//   chainer_maskrcnn/model/maskrcnn.py:231-246  (sigmoid, channel pick, cv2.resize to the box, threshold, paste)
// The arithmetic itself (decode row, candidate key and sort, suppression predicate, paste pixel rule) is detect_common.h's, shared with
// the multi-view kernels of tta.hip.  Latency-bound kernels (<= 300 RoIs, <= 80 classes).
#include "common.h"
#include "detect_common.h"

namespace {

// One thread per RoI: class-agnostic loc -> box in original-image pixels; softmax over the n_class scores.
__global__ __launch_bounds__(256) void k_detect_decode(const float *__restrict__ rois, int R, const float *__restrict__ box_out,
                                                       int ld, int n_class, int loc0, float scale, float4 mean, float4 stdv,
                                                       float size_h, float size_w, float *__restrict__ cls_bbox,
                                                       float *__restrict__ prob) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    *reinterpret_cast<float4 *>(cls_bbox + (size_t)i * 4) = detect_decode_row(
        rois + (size_t)i * 4, box_out + (size_t)i * ld, n_class, loc0, scale, mean, stdv, size_h, size_w, prob + (size_t)i * n_class);
}

// One workgroup per class l in [l_begin, l_end): the candidates of detect_common.h sorted, greedy NMS, everything in LDS.
// Output: keep_idx[l][0..cnt) = RoI indices in selection order.
__global__ __launch_bounds__(256) void k_class_nms(const float *__restrict__ cls_bbox, const float *__restrict__ prob, int R,
                                                   int n_class, int l_begin, float score_thresh, float nms_thresh,
                                                   int32_t *__restrict__ keep_idx, int32_t *__restrict__ keep_cnt) {
    __shared__ u64 skey[CN_CAP];
    __shared__ float4 sbox[CN_CAP];
    __shared__ u64 smask[CN_CAP][CN_CAP / 64];
    __shared__ int s_n;
    const int l = l_begin + blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < CN_CAP; i += 256) skey[i] = i < R ? candidate_key(prob[(size_t)i * n_class + l], score_thresh, i) : 0ull;
    __syncthreads();
    bitonic_sort_desc<256>(skey, CN_CAP, tid);
    if (tid == 0) {
        int n = 0;
        while (n < CN_CAP && skey[n] != 0ull) ++n;
        s_n = n;
    }
    __syncthreads();
    const int n = s_n;
    for (int i = tid; i < n; i += 256) sbox[i] = *reinterpret_cast<const float4 *>(cls_bbox + (size_t)candidate_index(skey[i]) * 4);
    __syncthreads();
    const int nw = (n + 63) / 64;
    for (int t = tid; t < n * nw; t += 256) {
        const int i = t / nw, wd = t % nw;
        const float4 b = sbox[i];
        const float area_i = (b.z - b.x) * (b.w - b.y);
        u64 bits = 0ull;
        for (int jj = 0; jj < 64; ++jj) {
            const int j = wd * 64 + jj;
            if (j >= n || j <= i) continue;
            if (nms_suppresses(b, area_i, sbox[j], nms_thresh)) bits |= 1ull << jj;
        }
        smask[i][wd] = bits;
    }
    __syncthreads();
    if (tid == 0) {           // n <= 512: the sequential sweep is a few microseconds
        u64 rem[CN_CAP / 64];
        for (int w = 0; w < CN_CAP / 64; ++w) rem[w] = 0ull;
        int cnt = 0;
        for (int i = 0; i < n; ++i) {
            if ((rem[i >> 6] >> (i & 63)) & 1ull) continue;
            keep_idx[(size_t)l * R + cnt++] = candidate_index(skey[i]);
            for (int w = 0; w < nw; ++w) rem[w] |= smask[i][w];
        }
        keep_cnt[l] = cnt;
    }
}

// Mask paste: mask_paste_box on m = sigmoid(logit[d, :, :, label[d]]).
__global__ __launch_bounds__(256) void k_mask_paste(const float *__restrict__ logits, int S, int Cm, const int32_t *__restrict__ label,
                                                    const float *__restrict__ bbox, int H, int W, unsigned char *__restrict__ out) {
    const int d = blockIdx.y;
    const float *lg = logits + (size_t)d * S * S * Cm + label[d];
    mask_paste_box(*reinterpret_cast<const float4 *>(bbox + (size_t)d * 4), S, H, W, out + (size_t)d * H * W,
                   [&](int yy, int xx) { return sigmoid1(lg[((size_t)yy * S + xx) * Cm]); });
}

}  // namespace

extern "C" int mrcnn_detect_decode_f32(const float *rois, int R, const float *box_out, int ld, int n_class, int loc0,
                                       float scale, const float *loc_mean4, const float *loc_std4, float size_h,
                                       float size_w, float *cls_bbox, float *prob, void *stream) {
    if (R == 0) return 0;
    if (!rois || !box_out || !loc_mean4 || !loc_std4 || !cls_bbox || !prob || R < 0 || n_class <= 0 || ld < loc0 + 4 || scale <= 0.f)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "detect_decode: bad arguments");
    hipLaunchKernelGGL(k_detect_decode, dim3(mrcnn::cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, rois, R, box_out, ld, n_class,
                       loc0, scale, make_float4(loc_mean4[0], loc_mean4[1], loc_mean4[2], loc_mean4[3]),
                       make_float4(loc_std4[0], loc_std4[1], loc_std4[2], loc_std4[3]), size_h, size_w, cls_bbox, prob);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_class_nms_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end,
                                   float score_thresh, float nms_thresh, int32_t *keep_idx, int32_t *keep_cnt, void *stream) {
    if (!cls_bbox || !prob || !keep_idx || !keep_cnt || R <= 0 || n_class <= 0 || l_begin < 0 || l_end > n_class || l_begin > l_end)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "class_nms: bad arguments");
    if (R > CN_CAP) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "class_nms: %d RoIs > %d", R, CN_CAP);
    MRCNN_HIP_TRY(hipMemsetAsync(keep_cnt, 0, sizeof(int32_t) * n_class, (hipStream_t)stream));
    if (l_end > l_begin) {
        hipLaunchKernelGGL(k_class_nms, dim3(l_end - l_begin), dim3(256), 0, (hipStream_t)stream, cls_bbox, prob, R, n_class, l_begin,
                           score_thresh, nms_thresh, keep_idx, keep_cnt);
        MRCNN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mrcnn_mask_paste_f32(const float *mask_logits, int D, int S, int Cm, const int32_t *label, const float *bbox,
                                    int H, int W, unsigned char *out, void *stream) {
    if (D == 0) return 0;
    if (!mask_logits || !label || !bbox || !out || D < 0 || S <= 0 || Cm <= 0 || H <= 0 || W <= 0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_paste: bad arguments");
    hipLaunchKernelGGL(k_mask_paste, dim3(std::min(mrcnn::cdiv((long long)H * W, 256), 1024), D), dim3(256), 0, (hipStream_t)stream,
                       mask_logits, S, Cm, label, bbox, H, W, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
