// Soft-NMS and box voting on gfx950: Detectron's TEST.SOFT_NMS (Bodla et al. 2017) and TEST.BBOX_VOTE on the decoded
// candidates of predict.hip / tta.hip, for the single view (R <= 300) and the union of the test-time views (R <= 4096).  The rules - the
// candidate test, the IoU (box_common.h nms_iou), the score weight - are detect_common.h's, shared with the hard NMS kernels.  Latency-bound kernels.
//   k_class_soft_nms  one workgroup per class.  The class's candidates (prob > score_thresh) are compacted in row order into three arrays
//                     (working score, row, box): in LDS for up to kLdsCap candidates, in the caller's workspace above.  Every trip of
//                     the loop selects one detection: the workgroup's arg-max over the packed keys valid | orderable(s) << 31 | slot
//                     (slots ascend with the rows, so the key order is the rule's (score, row) order) - a wave reduction, then one LDS
//                     step across the waves - and one pass in which every thread decays the scores of its own slots (slot % kT == its
//                     index) and takes their next local maximum.  One barrier per trip: the per-wave keys alternate between two LDS rows,
//                     a thread writes only its own slots, and the boxes are read-only after the compaction.  The loop ends at the
//                     first all-zero arg-max.
//   k_box_vote        one wave per (class, kept detection), grid-stride over the kept detections: the lanes sweep the rows in order,
//                     accumulate prob * box and prob of the rows that vote, and a fixed butterfly adds the lanes.  No atomics.
#include "common.h"
#include "detect_common.h"

namespace {

constexpr int kT = 256;                          // 4 waves
constexpr int kWaves = kT / kWave;
constexpr int kLdsCap = MRCNN_SOFT_NMS_LDS_MAX;  // candidates of a class held in LDS: 2048 * (4 + 4 + 16) bytes = 48 KiB
constexpr int kRMax = MRCNN_BOXPOST_MAX;
static_assert(SOFT_NMS_HARD == MRCNN_SOFT_NMS_HARD && SOFT_NMS_LINEAR == MRCNN_SOFT_NMS_LINEAR && SOFT_NMS_GAUSSIAN == MRCNN_SOFT_NMS_GAUSSIAN,
              "detect_common.h's methods are the public header's");
constexpr int kVoteBlocks = 64;                  // workgroups along the kept detections of a class

__device__ __forceinline__ float unorderable(unsigned u) {    // the inverse of orderable()
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

__device__ __forceinline__ u64 slot_key(float s, float score_thresh, int slot) {
    return s > score_thresh ? (1ull << 63) | ((u64)orderable(s) << 31) | (u64)slot : 0ull;
}

__device__ __forceinline__ u64 wave_max(u64 v) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const u64 w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// The selection loop of one class over the arrays sc / ix / bx (n slots are filled by this function; LDS or global memory).
__device__ __forceinline__ void soft_nms_class(float *sc, int *ix, float4 *bx, u64 (*s_wkey)[kWaves], int *s_wcnt,
                                               const float *__restrict__ cls_bbox, const float *__restrict__ prob, int R, int n_class, int l,
                                               float score_thresh, int method, float nms_thresh, float sigma,
                                               int32_t *__restrict__ keep_idx, float *__restrict__ keep_score, int32_t *__restrict__ keep_cnt) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    int n = 0;
    for (int i0 = 0; i0 < R; i0 += kT) {         // compaction, in row order
        const int i = i0 + tid;
        const float p = i < R ? prob[(size_t)i * n_class + l] : 0.f;
        const bool is = i < R && p > score_thresh;
        const u64 bal = __ballot(is);
        if (lane == 0) s_wcnt[wv] = __popcll(bal);
        __syncthreads();
        int off = n;
        for (int w = 0; w < kWaves; ++w) {
            const int c = s_wcnt[w];
            if (w < wv) off += c;
            n += c;
        }
        if (is) {
            const int slot = off + __popcll(bal & ((1ull << lane) - 1));
            sc[slot] = p;
            ix[slot] = i;
            bx[slot] = *reinterpret_cast<const float4 *>(cls_bbox + (size_t)i * 4);
        }
        __syncthreads();                         // s_wcnt is rewritten; after the last chunk: the slots are visible
    }
    u64 best = 0ull;
    for (int slot = tid; slot < n; slot += kT) {
        const u64 k = slot_key(sc[slot], score_thresh, slot);
        best = k > best ? k : best;
    }
    int cnt = 0, par = 0;
    for (;;) {
        const u64 wb = wave_max(best);
        if (lane == 0) s_wkey[par][wv] = wb;
        __syncthreads();
        u64 m = 0ull;
        for (int w = 0; w < kWaves; ++w) {
            const u64 k = s_wkey[par][w];
            m = k > m ? k : m;
        }
        par ^= 1;
        if (m == 0ull) break;                    // (the same in every thread)
        const int ms = (int)(m & 0x7FFFFFFFull);
        if (tid == 0) {
            keep_idx[(size_t)l * R + cnt] = ix[ms];
            keep_score[(size_t)l * R + cnt] = unorderable((unsigned)((m >> 31) & 0xFFFFFFFFull));
        }
        ++cnt;
        const float4 bm = bx[ms];
        const float area_m = (bm.z - bm.x) * (bm.w - bm.y);
        best = 0ull;
        for (int slot = tid; slot < n; slot += kT) {
            float s = sc[slot];
            if (!(s > score_thresh)) continue;   // removed earlier
            if (slot == ms) {
                sc[slot] = -INFINITY;
                continue;
            }
            const float w = soft_nms_weight(method, nms_iou(bm, area_m, bx[slot]), nms_thresh, sigma);
            if (w != 1.0f) {
                s = s * w;
                sc[slot] = s;
            }
            const u64 k = slot_key(s, score_thresh, slot);
            best = k > best ? k : best;
        }
    }
    if (tid == 0) keep_cnt[l] = cnt;
}

// grid (classes); ws: the boxes of all classes, then the scores, then the rows ((grid, R) each), used where a class has more than
// kLdsCap candidates
__global__ __launch_bounds__(kT) void k_class_soft_nms(const float *__restrict__ cls_bbox, const float *__restrict__ prob, int R, int n_class,
                                                      int l_begin, float score_thresh, int method, float nms_thresh, float sigma,
                                                      int32_t *__restrict__ keep_idx, float *__restrict__ keep_score,
                                                      int32_t *__restrict__ keep_cnt, void *ws) {
    __shared__ float4 s_bx[kLdsCap];
    __shared__ float s_sc[kLdsCap];
    __shared__ int s_ix[kLdsCap];
    __shared__ u64 s_wkey[2][kWaves];
    __shared__ int s_wcnt[kWaves];
    const int l = l_begin + blockIdx.x, tid = threadIdx.x;
    int c = 0;
    for (int i = tid; i < R; i += kT) c += prob[(size_t)i * n_class + l] > score_thresh ? 1 : 0;
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & (kWave - 1)) == 0) s_wcnt[tid / kWave] = c;
    __syncthreads();
    int n = 0;
    for (int w = 0; w < kWaves; ++w) n += s_wcnt[w];
    __syncthreads();                             // s_wcnt is rewritten by the compaction
    if (n <= kLdsCap) {
        soft_nms_class(s_sc, s_ix, s_bx, s_wkey, s_wcnt, cls_bbox, prob, R, n_class, l, score_thresh, method, nms_thresh, sigma, keep_idx,
                       keep_score, keep_cnt);
    } else {                                     // only where R > kLdsCap: the host has checked the workspace
        const size_t rows = (size_t)gridDim.x * R, at = (size_t)blockIdx.x * R;
        float4 *g_bx = reinterpret_cast<float4 *>(ws);
        float *g_sc = reinterpret_cast<float *>(g_bx + rows);
        int *g_ix = reinterpret_cast<int *>(g_sc + rows);
        soft_nms_class(g_sc + at, g_ix + at, g_bx + at, s_wkey, s_wcnt, cls_bbox, prob, R, n_class, l, score_thresh, method, nms_thresh, sigma,
                       keep_idx, keep_score, keep_cnt);
    }
}

// grid (kVoteBlocks, classes): wave w of workgroup g takes the kept detections k = g * kWaves + w, + kVoteBlocks * kWaves, ...
__global__ __launch_bounds__(kT) void k_box_vote(const float *__restrict__ cls_bbox, const float *__restrict__ prob, int R, int n_class,
                                                int l_begin, float score_thresh, float vote_thresh, const int32_t *__restrict__ keep_idx,
                                                const int32_t *__restrict__ keep_cnt, float *__restrict__ keep_box) {
    const int l = l_begin + blockIdx.y, lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int cnt = min(max(keep_cnt[l], 0), R);
    for (int k = blockIdx.x * kWaves + wv; k < cnt; k += gridDim.x * kWaves) {
        const int ik = keep_idx[(size_t)l * R + k];
        if (ik < 0 || ik >= R) continue;         // not an index of this input: the row is left unwritten
        const float4 b = *reinterpret_cast<const float4 *>(cls_bbox + (size_t)ik * 4);
        const float area = (b.z - b.x) * (b.w - b.y);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, ws = 0.f;
        int nv = 0;
        for (int i = lane; i < R; i += kWave) {
            const float p = prob[(size_t)i * n_class + l];
            if (!(p > score_thresh)) continue;
            const float4 c = *reinterpret_cast<const float4 *>(cls_bbox + (size_t)i * 4);
            if (!(nms_iou(b, area, c) >= vote_thresh)) continue;
            a0 += p * c.x; a1 += p * c.y; a2 += p * c.z; a3 += p * c.w;
            ws += p;
            ++nv;
        }
        for (int o = kWave / 2; o > 0; o >>= 1) {
            a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); a3 += __shfl_xor(a3, o);
            ws += __shfl_xor(ws, o);
            nv += __shfl_xor(nv, o);
        }
        if (lane == 0)
            *reinterpret_cast<float4 *>(keep_box + ((size_t)l * R + k) * 4) = nv > 0 ? make_float4(a0 / ws, a1 / ws, a2 / ws, a3 / ws) : b;
    }
}

const char *range_error(const void *cls_bbox, const void *prob, int R, int n_class, int l_begin, int l_end) {
    if (R <= 0) return "R is not positive";
    if (n_class <= 0) return "n_class is not positive";
    if (l_begin < 0 || l_end > n_class || l_begin > l_end) return "the l range lies outside [0, n_class]";
    if (!cls_bbox) return "cls_bbox is NULL";
    if (!prob) return "prob is NULL";
    if (reinterpret_cast<uintptr_t>(cls_bbox) & 15) return "cls_bbox is not 16-byte aligned";
    if (reinterpret_cast<uintptr_t>(prob) & 3) return "prob is not 4-byte aligned";
    return nullptr;
}

}  // namespace

extern "C" size_t mrcnn_class_soft_nms_workspace_bytes(int R, int n_class) {
    if (R <= kLdsCap || R > kRMax || n_class <= 0) return 0;
    return (size_t)n_class * R * (sizeof(float4) + sizeof(float) + sizeof(int));
}

extern "C" int mrcnn_class_soft_nms_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end,
                                        float score_thresh, int method, float nms_thresh, float sigma, int32_t *keep_idx, float *keep_score,
                                        int32_t *keep_cnt, void *ws, size_t ws_bytes, void *stream) {
    if (R > kRMax) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "class_soft_nms: %d RoIs > %d", R, kRMax);
    if (const char *e = range_error(cls_bbox, prob, R, n_class, l_begin, l_end)) return mrcnn::fail_arg(MRCNN_E_INVALID, "class_soft_nms: %s", e);
    if (method != MRCNN_SOFT_NMS_HARD && method != MRCNN_SOFT_NMS_LINEAR && method != MRCNN_SOFT_NMS_GAUSSIAN)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "class_soft_nms: unknown method %d", method);
    if (!(sigma > 0.f)) return mrcnn::fail_arg(MRCNN_E_INVALID, "class_soft_nms: sigma %g is not positive", (double)sigma);
    if (!keep_idx || !keep_score || !keep_cnt) return mrcnn::fail_arg(MRCNN_E_INVALID, "class_soft_nms: keep_idx, keep_score or keep_cnt is NULL");
    if ((reinterpret_cast<uintptr_t>(keep_idx) | reinterpret_cast<uintptr_t>(keep_score) | reinterpret_cast<uintptr_t>(keep_cnt)) & 3)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "class_soft_nms: keep_idx, keep_score or keep_cnt is not 4-byte aligned");
    const size_t need = mrcnn_class_soft_nms_workspace_bytes(R, n_class);
    if (need) {
        if (!ws || ws_bytes < need) return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "class_soft_nms: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
        if (reinterpret_cast<uintptr_t>(ws) & 15) return mrcnn::fail_arg(MRCNN_E_INVALID, "class_soft_nms: workspace not 16-byte aligned");
    }
    MRCNN_HIP_TRY(hipMemsetAsync(keep_cnt, 0, sizeof(int32_t) * n_class, (hipStream_t)stream));
    if (l_end > l_begin) {
        hipLaunchKernelGGL(k_class_soft_nms, dim3(l_end - l_begin), dim3(kT), 0, (hipStream_t)stream, cls_bbox, prob, R, n_class, l_begin,
                           score_thresh, method, nms_thresh, sigma, keep_idx, keep_score, keep_cnt, ws);
        MRCNN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mrcnn_box_vote_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end, float score_thresh,
                                  float vote_thresh, const int32_t *keep_idx, const int32_t *keep_cnt, float *keep_box, void *stream) {
    if (R > kRMax) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "box_vote: %d RoIs > %d", R, kRMax);
    if (const char *e = range_error(cls_bbox, prob, R, n_class, l_begin, l_end)) return mrcnn::fail_arg(MRCNN_E_INVALID, "box_vote: %s", e);
    if (!(score_thresh >= 0.f))       // every voter then has prob > 0: a vote set that is not empty has a positive weight sum
        return mrcnn::fail_arg(MRCNN_E_INVALID, "box_vote: score_thresh %g is negative", (double)score_thresh);
    if (!(vote_thresh > 0.f && vote_thresh <= 1.f))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "box_vote: vote_thresh %g outside (0, 1]", (double)vote_thresh);
    if (!keep_idx || !keep_cnt || !keep_box) return mrcnn::fail_arg(MRCNN_E_INVALID, "box_vote: keep_idx, keep_cnt or keep_box is NULL");
    if ((reinterpret_cast<uintptr_t>(keep_idx) | reinterpret_cast<uintptr_t>(keep_cnt)) & 3)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "box_vote: keep_idx or keep_cnt is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(keep_box) & 15) return mrcnn::fail_arg(MRCNN_E_INVALID, "box_vote: keep_box is not 16-byte aligned");
    if (l_end > l_begin) {
        hipLaunchKernelGGL(k_box_vote, dim3(std::min(mrcnn::cdiv(R, kWaves), kVoteBlocks), l_end - l_begin), dim3(kT), 0, (hipStream_t)stream,
                           cls_bbox, prob, R, n_class, l_begin, score_thresh, vote_thresh, keep_idx, keep_cnt, keep_box);
        MRCNN_LAUNCH_CHECK();
    }
    return 0;
}
