// Test-time augmentation (TTA) post-processing for gfx950 (MaskRCNN.use_test_augmentation): every image runs at
// several short sides, optionally mirrored, one N = 1 forward per view; the kernels here merge the views after the forward pass.
//   multi-view decode      detect_decode_row per view (scale_v), mirrored views mapped back to (y1, W-x2, y2, W-x1)
//   union class NMS        R <= 4096 candidates: per class an LDS bitonic sort, an IoU bitmask in the caller's workspace, a one-wave sweep
//   mask merge + paste     mean over the views of sigmoid(logit) at the mirrored column, then mask_paste_box's resize / threshold rule
//   keypoint merge         mean over the views of the heat maps, mirrored column and left / right channels swapped
// The decode row, the candidate key and sort, the suppression predicate and the paste pixel rule are detect_common.h's, the functions
// predict.hip's single-view kernels call, so one unmirrored view gives predict()'s bits.  The views' mirrored resize is nn.hip's
// k_image_resize_mirror_f32.
#include "common.h"
#include "detect_common.h"

namespace {

constexpr int NT = 256;
constexpr int UNION_MAX = MRCNN_CLASS_NMS_WS_MAX;

// ---- multi-view decode ------------------------------------------------------------------------------------------------------------------
struct DecodeViews {
    const float *rois[MRCNN_TTA_VIEWS_MAX];
    const float *box[MRCNN_TTA_VIEWS_MAX];
    int off[MRCNN_TTA_VIEWS_MAX + 1];            // first union row of each view; off[V] = R
    int mirror[MRCNN_TTA_VIEWS_MAX];
    float scale[MRCNN_TTA_VIEWS_MAX];
};

// One thread per union row: detect_decode_row with the row's view's scale, then the mirror back.
__global__ __launch_bounds__(NT) void k_tta_detect_decode(const DecodeViews vs, int V, int ld, int n_class, int loc0, float4 mean, float4 stdv,
                                                          float size_h, float size_w, float *__restrict__ cls_bbox, float *__restrict__ prob) {
    const int g = blockIdx.x * NT + threadIdx.x;
    if (g >= vs.off[V]) return;
    int v = 0;
    while (g >= vs.off[v + 1]) ++v;
    const int i = g - vs.off[v];
    float4 b = detect_decode_row(vs.rois[v] + (size_t)i * 4, vs.box[v] + (size_t)i * ld, n_class, loc0, vs.scale[v], mean, stdv, size_h,
                                 size_w, prob + (size_t)g * n_class);
    if (vs.mirror[v]) b = make_float4(b.x, size_w - b.w, b.z, size_w - b.y);
    *reinterpret_cast<float4 *>(cls_bbox + (size_t)g * 4) = b;
}

// ---- union class NMS (R <= 4096) --------------------------------------------------------------------------------------------------------
struct UnionLayout {
    size_t sboxes, sidx, n_valid, mask, total;
    int nblk;
};
size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
UnionLayout union_layout(int R, int n_class) {
    UnionLayout L;
    L.nblk = (R + 63) / 64;
    size_t o = 0;
    L.sboxes = o;  o = al256(o + (size_t)n_class * R * 16);
    L.sidx = o;    o = al256(o + (size_t)n_class * R * 4);
    L.n_valid = o; o = al256(o + (size_t)n_class * 4);
    L.mask = o;    o = al256(o + (size_t)n_class * R * L.nblk * 8);
    L.total = o;
    return L;
}

// One workgroup per class l: the candidate keys (prob > thresh; score descending, then index descending) bitonic-sorted in LDS over
// P = pow2 >= R; the n candidates' boxes and indices in sort order go to the workspace.  Slot s = l - l_begin.
constexpr int SORT_T = 1024;
__global__ __launch_bounds__(SORT_T) void k_union_sort(const float *__restrict__ cls_bbox, const float *__restrict__ prob, int R, int P,
                                                      int n_class, int l_begin, float score_thresh, float4 *__restrict__ sboxes,
                                                      int32_t *__restrict__ sidx, int32_t *__restrict__ n_valid) {
    __shared__ u64 skey[UNION_MAX];
    __shared__ int s_n;
    const int s = blockIdx.x, l = l_begin + s, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    int mine = 0;
    for (int i = tid; i < P; i += SORT_T) {
        const u64 k = i < R ? candidate_key(prob[(size_t)i * n_class + l], score_thresh, i) : 0ull;
        mine += k != 0ull;
        skey[i] = k;
    }
    __syncthreads();
    if (mine) atomicAdd(&s_n, mine);
    bitonic_sort_desc<SORT_T>(skey, P, tid);
    const int n = s_n;
    for (int i = tid; i < n; i += SORT_T) {
        const int idx = candidate_index(skey[i]);
        sboxes[(size_t)s * R + i] = *reinterpret_cast<const float4 *>(cls_bbox + (size_t)idx * 4);
        sidx[(size_t)s * R + i] = idx;
    }
    if (tid == 0) n_valid[s] = n;
}

// mask[(s*R + i)*nblk + cb] bit j: sorted box i suppresses sorted box cb*64+j (> i) by nms_suppresses, as in k_class_nms.
// Grid (nblk, cdiv(nblk, 4), classes), 4 waves = 4 row blocks; only words cb >= rb are written, the only ones the sweep reads.
__global__ __launch_bounds__(256) void k_union_mask(const float4 *__restrict__ sboxes, const int32_t *__restrict__ n_valid, int R, int nblk,
                                                    float thresh, u64 *__restrict__ mask) {
    const int s = blockIdx.z, cb = blockIdx.x;
    const int n = n_valid[s];
    if (cb * 64 >= n || blockIdx.y * 256 >= n || (int)blockIdx.y * 4 > cb) return;
    __shared__ float4 cbox[64];
    const float4 *bx = sboxes + (size_t)s * R;
    const int lane = threadIdx.x & 63, rb = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (threadIdx.x < 64) {
        const int cj = cb * 64 + lane;
        cbox[lane] = cj < n ? bx[cj] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int i = rb * 64 + lane;
    if (rb > cb || i >= n) return;
    const float4 b = bx[i];
    const float area_i = (b.z - b.x) * (b.w - b.y);
    u64 bits = 0ull;
    const int jmax = min(64, n - cb * 64);
    for (int j = 0; j < jmax; ++j)
        if (nms_suppresses(b, area_i, cbox[j], thresh) && cb * 64 + j > i) bits |= 1ull << j;
    mask[((size_t)s * R + i) * nblk + cb] = bits;
}

// One wave per class: the greedy sweep over the sorted candidates, 64 at a time.  Lane w holds word w of the removed set (nblk <= 64).
// Inside a chunk only boxes whose diagonal word is non-zero can remove a later box of the chunk; they are visited in order.  The kept
// boxes' rows then go into the later words, 8 independent loads at a time.
__global__ __launch_bounds__(64) void k_union_sweep(const u64 *__restrict__ mask, const int32_t *__restrict__ sidx,
                                                    const int32_t *__restrict__ n_valid, int R, int nblk, int l_begin,
                                                    int32_t *__restrict__ keep_idx, int32_t *__restrict__ keep_cnt) {
    const int s = blockIdx.x, l = l_begin + s, lane = threadIdx.x;
    const int n = n_valid[s];
    const int nb = (n + 63) / 64;
    const u64 *mk = mask + (size_t)s * R * nblk;
    const int32_t *si = sidx + (size_t)s * R;
    int32_t *kp = keep_idx + (size_t)l * R;
    u64 rem = 0ull;
    int cnt = 0;
    for (int c = 0; c < nb; ++c) {
        const int box = c * 64 + lane;
        const u64 diag = box < n ? mk[(size_t)box * nblk + c] : 0ull;
        const u64 remc = __shfl(rem, c, 64);
        u64 alive = ~remc;
        const int m = min(64, n - c * 64);
        if (m < 64) alive &= (1ull << m) - 1ull;
        u64 pend = alive & __ballot(diag != 0ull);
        while (pend) {
            const int b = __builtin_ctzll(pend);
            const u64 Db = __shfl(diag, b, 64);
            alive &= ~Db;
            pend &= ~Db;
            pend &= ~(1ull << b);
        }
        if ((alive >> lane) & 1ull) kp[cnt + __popcll(alive & ((1ull << lane) - 1ull))] = si[box];
        cnt += __popcll(alive);
        if (c + 1 < nb) {
            const bool mine = lane > c && lane < nb;
            u64 acc = 0ull, left = alive;
            while (left) {
                int bs[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    bs[q] = left ? __builtin_ctzll(left) : -1;
                    if (left) left &= left - 1ull;
                }
                u64 v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = (mine && bs[q] >= 0) ? mk[(size_t)(c * 64 + bs[q]) * nblk + lane] : 0ull;
#pragma unroll
                for (int q = 0; q < 8; ++q) acc |= v[q];
            }
            rem |= acc;
        }
    }
    if (lane == 0) keep_cnt[l] = cnt;
}

// ---- mask merge + paste -----------------------------------------------------------------------------------------------------------------
struct MergeViews {
    const float *src[MRCNN_TTA_VIEWS_MAX];
    int mirror[MRCNN_TTA_VIEWS_MAX];
};

// prob[d, y, x] = (sum over views u, in order, of sigmoid(logits_u[d, y, x_u, label[d]])) / V; x_u = S-1-x for a mirrored view.
__global__ __launch_bounds__(NT) void k_tta_mask_merge(const MergeViews vs, int V, int D, int S, int Cm, const int32_t *__restrict__ label,
                                                       float *__restrict__ prob) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= D * S * S) return;
    const int d = i / (S * S), yx = i - d * S * S, y = yx / S, x = yx - y * S;
    const int ch = label[d];
    float acc = 0.f;
    for (int u = 0; u < V; ++u) {
        const int xu = vs.mirror[u] ? S - 1 - x : x;
        const float z = vs.src[u][(((size_t)d * S + y) * S + xu) * Cm + ch];
        const float p = sigmoid1(z);
        acc = u == 0 ? p : acc + p;
    }
    prob[i] = acc / (float)V;
}

// Mask paste: mask_paste_box on the stored probabilities m = prob[d].
__global__ __launch_bounds__(256) void k_mask_paste_prob(const float *__restrict__ prob, int S, const float *__restrict__ bbox, int H, int W,
                                                         unsigned char *__restrict__ out) {
    const int d = blockIdx.y;
    const float *pr = prob + (size_t)d * S * S;
    mask_paste_box(*reinterpret_cast<const float4 *>(bbox + (size_t)d * 4), S, H, W, out + (size_t)d * H * W,
                   [&](int yy, int xx) { return pr[(size_t)yy * S + xx]; });
}

// ---- keypoint heat-map merge ------------------------------------------------------------------------------------------------------------
struct KpViews {
    const float *src[MRCNN_TTA_VIEWS_MAX];
    int mirror[MRCNN_TTA_VIEWS_MAX];
    unsigned char perm[MRCNN_TTA_KEYPOINTS_MAX];
};

// out[d, y, x, k] = (sum over views u, in order, of heat_u[d, y, x_u, k_u]) / V; mirrored view: x_u = S-1-x, k_u = perm[k] for k < K.
__global__ __launch_bounds__(NT) void k_tta_keypoint_merge(const KpViews vs, int V, int D, int S, int Cp, int K, float *__restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= D * S * S * Cp) return;
    const int k = i % Cp, pix = i / Cp;
    const int x = pix % S;
    const size_t row = (size_t)(pix - x);                // (d * S + y) * S
    float acc = 0.f;
    for (int u = 0; u < V; ++u) {
        const bool mr = vs.mirror[u] != 0;
        const int xu = mr ? S - 1 - x : x;
        const int ku = (mr && k < K) ? (int)vs.perm[k] : k;
        const float h = vs.src[u][(row + xu) * Cp + ku];
        acc = u == 0 ? h : acc + h;
    }
    out[i] = acc / (float)V;
}

int check_views(const char *who, const mrcnn_tta_view_t *views, int V) {
    if (!views) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: null view table", who);
    if (V < 1 || V > MRCNN_TTA_VIEWS_MAX) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: V = %d outside 1..%d", who, V, MRCNN_TTA_VIEWS_MAX);
    for (int v = 0; v < V; ++v)
        if (views[v].mirror != 0 && views[v].mirror != 1)
            return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: view %d has mirror %d (0 or 1 expected)", who, v, views[v].mirror);
    return 0;
}

}  // namespace

extern "C" int mrcnn_tta_detect_decode_f32(const float *const *rois, const float *const *box_out, const mrcnn_tta_view_t *views, int V,
                                           int ld, int n_class, int loc0, const float *loc_mean4, const float *loc_std4, float size_h,
                                           float size_w, float *cls_bbox, float *prob, void *stream) {
    if (int e = check_views("tta_detect_decode", views, V)) return e;
    if (!rois || !box_out || !loc_mean4 || !loc_std4 || n_class <= 0 || loc0 < 0 || ld < loc0 + 4 || ld < n_class || !(size_h > 0.f) ||
        !(size_w > 0.f))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_detect_decode: bad arguments");
    DecodeViews vs = {};
    long long R = 0;
    for (int v = 0; v < V; ++v) {
        const mrcnn_tta_view_t &w = views[v];
        if (w.R < 0 || !(w.scale > 0.f) || (w.R > 0 && (!rois[v] || !box_out[v])))
            return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_detect_decode: bad view %d (R %d, scale %g)", v, w.R, (double)w.scale);
        vs.rois[v] = rois[v];
        vs.box[v] = box_out[v];
        vs.mirror[v] = w.mirror;
        vs.scale[v] = w.scale;
        vs.off[v] = (int)R;
        R += w.R;
        if (R > 0x7FFFFF00LL) return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_detect_decode: %lld rows", R);
    }
    vs.off[V] = (int)R;
    if (R == 0) return 0;
    if (!cls_bbox || !prob) return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_detect_decode: null output");
    hipLaunchKernelGGL(k_tta_detect_decode, dim3(mrcnn::cdiv(R, NT)), dim3(NT), 0, (hipStream_t)stream, vs, V, ld, n_class, loc0,
                       make_float4(loc_mean4[0], loc_mean4[1], loc_mean4[2], loc_mean4[3]),
                       make_float4(loc_std4[0], loc_std4[1], loc_std4[2], loc_std4[3]), size_h, size_w, cls_bbox, prob);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mrcnn_class_nms_workspace_bytes(int R, int n_class) {
    if (R <= CN_CAP || R > UNION_MAX || n_class <= 0) return 0;
    return union_layout(R, n_class).total;
}

extern "C" int mrcnn_class_nms_ws_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end,
                                      float score_thresh, float nms_thresh, int32_t *keep_idx, int32_t *keep_cnt, void *ws, size_t ws_bytes,
                                      void *stream) {
    if (!cls_bbox || !prob || !keep_idx || !keep_cnt || R <= 0 || n_class <= 0 || l_begin < 0 || l_end > n_class || l_begin > l_end)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "class_nms_ws: bad arguments");
    if (R > UNION_MAX) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "class_nms_ws: %d RoIs > %d", R, UNION_MAX);
    if (R <= CN_CAP)           // the single-view kernel: one workgroup per class, everything in LDS
        return mrcnn_class_nms_f32(cls_bbox, prob, R, n_class, l_begin, l_end, score_thresh, nms_thresh, keep_idx, keep_cnt, stream);
    const UnionLayout L = union_layout(R, n_class);
    if (!ws || ws_bytes < L.total)
        return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "class_nms_ws: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    if (reinterpret_cast<uintptr_t>(ws) & 255) return mrcnn::fail_arg(MRCNN_E_INVALID, "class_nms_ws: workspace not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    MRCNN_HIP_TRY(hipMemsetAsync(keep_cnt, 0, sizeof(int32_t) * n_class, st));
    const int nc = l_end - l_begin;
    if (nc == 0) return 0;
    char *w = static_cast<char *>(ws);
    float4 *sboxes = reinterpret_cast<float4 *>(w + L.sboxes);
    int32_t *sidx = reinterpret_cast<int32_t *>(w + L.sidx), *n_valid = reinterpret_cast<int32_t *>(w + L.n_valid);
    u64 *mask = reinterpret_cast<u64 *>(w + L.mask);
    int P = 64;
    while (P < R) P <<= 1;
    hipLaunchKernelGGL(k_union_sort, dim3(nc), dim3(SORT_T), 0, st, cls_bbox, prob, R, P, n_class, l_begin, score_thresh, sboxes, sidx, n_valid);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_union_mask, dim3(L.nblk, (L.nblk + 3) / 4, nc), dim3(256), 0, st, sboxes, n_valid, R, L.nblk, nms_thresh, mask);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_union_sweep, dim3(nc), dim3(64), 0, st, mask, sidx, n_valid, R, L.nblk, l_begin, keep_idx, keep_cnt);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_tta_mask_merge_f32(const float *const *mask_logits, const mrcnn_tta_view_t *views, int V, int D, int S, int Cm,
                                        const int32_t *label, float *prob, void *stream) {
    if (int e = check_views("tta_mask_merge", views, V)) return e;
    if (D < 0 || S <= 0 || Cm <= 0 || (long long)D * S * S > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_mask_merge: bad sizes (D %d, S %d, Cm %d)", D, S, Cm);
    if (D == 0) return 0;
    if (!mask_logits || !label || !prob) return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_mask_merge: null pointer");
    MergeViews vs = {};
    for (int v = 0; v < V; ++v) {
        if (!mask_logits[v]) return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_mask_merge: null logits of view %d", v);
        vs.src[v] = mask_logits[v];
        vs.mirror[v] = views[v].mirror;
    }
    hipLaunchKernelGGL(k_tta_mask_merge, dim3(mrcnn::cdiv((long long)D * S * S, NT)), dim3(NT), 0, (hipStream_t)stream, vs, V, D, S, Cm,
                       label, prob);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_mask_paste_prob_f32(const float *prob, int D, int S, const float *bbox, int H, int W, unsigned char *out, void *stream) {
    if (D < 0 || S <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_paste_prob: bad sizes");
    if (D == 0) return 0;
    if (!prob || !bbox || !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_paste_prob: null pointer");
    if (D > 65535) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "mask_paste_prob: D = %d > 65535", D);
    if (reinterpret_cast<uintptr_t>(bbox) & 15) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_paste_prob: bbox not 16-byte aligned");
    hipLaunchKernelGGL(k_mask_paste_prob, dim3(std::min(mrcnn::cdiv((long long)H * W, 256), 1024), D), dim3(256), 0, (hipStream_t)stream,
                       prob, S, bbox, H, W, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_tta_keypoint_merge_f32(const float *const *heat, const mrcnn_tta_view_t *views, int V, int D, int S, int Cp, int K,
                                            const int32_t *perm, float *out, void *stream) {
    if (int e = check_views("tta_keypoint_merge", views, V)) return e;
    if (D < 0 || S <= 0 || K <= 0 || Cp < K || (long long)D * S * S * Cp > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_keypoint_merge: bad sizes (D %d, S %d, Cp %d, K %d)", D, S, Cp, K);
    if (K > MRCNN_TTA_KEYPOINTS_MAX) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "tta_keypoint_merge: K = %d > %d", K, MRCNN_TTA_KEYPOINTS_MAX);
    KpViews vs = {};
    bool any_mirror = false;
    for (int v = 0; v < V; ++v) any_mirror |= views[v].mirror != 0;
    if (any_mirror) {
        if (!perm) return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_keypoint_merge: a mirrored view needs the channel permutation");
        bool seen[MRCNN_TTA_KEYPOINTS_MAX] = {};
        for (int k = 0; k < K; ++k) {
            if (perm[k] < 0 || perm[k] >= K || seen[perm[k]])
                return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_keypoint_merge: perm is not a permutation of 0..%d (entry %d)", K - 1, k);
            seen[perm[k]] = true;
            vs.perm[k] = (unsigned char)perm[k];
        }
    }
    if (D == 0) return 0;
    if (!heat || !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_keypoint_merge: null pointer");
    for (int v = 0; v < V; ++v) {
        if (!heat[v]) return mrcnn::fail_arg(MRCNN_E_INVALID, "tta_keypoint_merge: null heat maps of view %d", v);
        vs.src[v] = heat[v];
        vs.mirror[v] = views[v].mirror;
    }
    hipLaunchKernelGGL(k_tta_keypoint_merge, dim3(mrcnn::cdiv((long long)D * S * S * Cp, NT)), dim3(NT), 0, (hipStream_t)stream, vs, V, D, S, Cp, K, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
