// Mask Scoring R-CNN (Huang et al., CVPR 2019) on the device for gfx950: the MaskIoU head's regression target, the assembly of its input
// and that assembly's backward, its masked L2 loss and the rescoring of the detections.  No counterpart in the
// reference, whose detections are ranked by the box score alone.
//   mrcnn_maskiou_target      ground-truth masks + sampled RoIs + mask logits -> the IoU every mask row should regress, two launches
//   mrcnn_maskiou_input_fwd   pooled features + 2x2/2 max of the class logit -> the head's input, one launch
//   mrcnn_maskiou_input_bwd   the head's input gradient added into the mask branch's pooled gradient, one launch
//   mrcnn_maskiou_l2          0.5 (x - t)^2 over the rows with a target, as a (sum, count) row of loss.hip's form
//   mrcnn_maskiou_rescore     score * clamp(predicted IoU, 0, 1), one launch
// Every count is an exact integer; nothing is added with float atomics, so two runs give the same bits.  Restated in NumPy by
// tests/maskiou_reference.py.
//
// The target of mask row r (image i = r / rows, sampler row i * n_sample + r % rows), in float32 with FP contraction off:
//   full     nonzero bytes of the assigned ground-truth mask over the whole image (k_mask_area: 0 for slots at or beyond n_gt[i])
//   crop     nonzero bytes of it inside the rectangle k_mask_target (targets.hip) crops: y0 = max((int)y1f, 0), y1 = min((int)y2f, H), x alike
//   pred     positions of the 28x28 map whose logit at channel label - label_base is > 0
//   gt28     positions with gt_roi_mask > 0;  ovr: positions where both hold
//   full_est = ((float)gt28 * (float)full) / (float)crop      the 28x28 target's area scaled up to the part of the mask outside the RoI
//   uni      = ((float)pred + full_est) - (float)ovr
//   target   = (float)ovr / fmaxf(uni, 1.0f)
// and 0 where crop == 0, full == 0, the RoI has no integer extent, or the row is padding (r % rows >= n_pos[i], channel outside
// [0, n_channels), no assignment below n_gt[i]).
#include "common.h"
#include "loss_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MI_CHUNKS = 32;      // workgroups per ground-truth mask in the area pass: 32 KiB each at 1024 x 1024

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// nonzero bytes of a 32-bit word: every byte's bits are or-ed down into its bit 0 (the shifts only ever move a byte's own higher bits there)
__device__ __forceinline__ int nz_bytes(unsigned w) {
    w |= w >> 4;
    w |= w >> 2;
    w |= w >> 1;
    return __popc(w & 0x01010101u);
}

// block-level sum of NV ints per thread of a THREADS-wide workgroup; the totals are valid in thread 0
template <int NV, int THREADS>
__device__ __forceinline__ void block_sum_i(int (&v)[NV]) {
    __shared__ int sm[THREADS / 64][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum_i(v[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) sm[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            int s = 0;
            for (int w = 0; w < THREADS / 64; ++w) s += sm[w][k];
            v[k] = s;
        }
}

// (a) Full areas.  grid (MI_CHUNKS, G, N): chunk c of mask (i, g) counts its share of the mask's 16-byte vectors - the mask starts at
// byte (i * G + g) * H * W of the buffer, so up to 15 head bytes in front of the first aligned vector and up to 15 tail bytes behind the
// last one are counted byte by byte, by chunk 0.  Lanes reduce in the wave, waves in LDS, and one int goes to part[(i * G + g) * MI_CHUNKS
// + c]; slots at or beyond n_gt[i] write 0 without reading the mask.
__global__ __launch_bounds__(NT) void k_mask_area(const unsigned char *__restrict__ masks, int G, long long HW,
                                                  const int32_t *__restrict__ n_gt, int32_t *__restrict__ part) {
    const int c = blockIdx.x, g = blockIdx.y, img = blockIdx.z;
    int32_t *o = part + ((size_t)img * G + g) * MI_CHUNKS + c;
    if (g >= n_gt[img]) {
        if (threadIdx.x == 0) *o = 0;
        return;
    }
    const unsigned char *p = masks + ((size_t)img * G + g) * (size_t)HW;
    const long long to16 = (long long)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15);
    const long long head = to16 < HW ? to16 : HW;
    const long long nvec = (HW - head) / 16, tail0 = head + nvec * 16;
    const long long per = (nvec + MI_CHUNKS - 1) / MI_CHUNKS;
    const long long v0 = (long long)c * per < nvec ? (long long)c * per : nvec, v1 = v0 + per < nvec ? v0 + per : nvec;
    const uint4 *pv = reinterpret_cast<const uint4 *>(p + head);
    int cnt[1] = {0};
    for (long long v = v0 + threadIdx.x; v < v1; v += NT) {
        const uint4 q = pv[v];
        cnt[0] += nz_bytes(q.x) + nz_bytes(q.y) + nz_bytes(q.z) + nz_bytes(q.w);
    }
    if (c == 0) {       // head [0, head) and tail [tail0, HW): fewer than 16 bytes each
        const long long t = threadIdx.x;
        if (t < head) cnt[0] += p[t] != 0;
        else if (t >= 16 && tail0 + (t - 16) < HW) cnt[0] += p[tail0 + (t - 16)] != 0;
    }
    block_sum_i<1, NT>(cnt);
    if (threadIdx.x == 0) *o = cnt[0];
}

// (b) One workgroup of TB threads per mask row; workgroups at and beyond Rm add the area partials into area (N, G), TB masks each.
// The crop count walks the rectangle a line per 16 lanes: the line's bytes [x0, x1) as 16-byte vectors between a byte-wise head (up to the
// first 16-byte boundary) and tail, every load inside the rectangle.
constexpr int TB = 512;

__global__ __launch_bounds__(TB) void k_maskiou_target(
    const unsigned char *__restrict__ masks, int N, int G, int H, int W, const int32_t *__restrict__ n_gt,
    const int32_t *__restrict__ part, int32_t *__restrict__ area,
    const float *__restrict__ sample_roi, const int32_t *__restrict__ gt_assign, const int32_t *__restrict__ label,
    const int32_t *__restrict__ n_pos, int n_sample, int rows, int Rm, const float *__restrict__ mask_out, int msz, int Cp,
    int n_channels, const int32_t *__restrict__ gt_roi_mask, int label_base, float *__restrict__ target, int32_t *__restrict__ counts) {
    if ((int)blockIdx.x >= Rm) {
        const int m = ((int)blockIdx.x - Rm) * TB + threadIdx.x;
        if (m < N * G) {
            int s = 0;
            for (int c = 0; c < MI_CHUNKS; ++c) s += part[(size_t)m * MI_CHUNKS + c];
            area[m] = s;
        }
        return;
    }
    const int r = blockIdx.x, img = r / rows, j = r % rows;
    const int srow = img * n_sample + j;
    const int ch = label[r] - label_base;
    const int g = gt_assign[srow];
    const bool live = j < n_pos[img] && ch >= 0 && ch < n_channels && g >= 0 && g < G && g < n_gt[img];
    int v[4] = {0, 0, 0, 0};        // crop, pred, gt28, ovr
    int full = 0;
    if (live) {
        for (int c = 0; c < MI_CHUNKS; ++c) full += part[((size_t)img * G + g) * MI_CHUNKS + c];
        const float4 b = *reinterpret_cast<const float4 *>(sample_roi + (size_t)srow * 4);
        const int y0 = max((int)b.x, 0), y1 = min((int)b.z, H), x0 = max((int)b.y, 0), x1 = min((int)b.w, W);
        const unsigned char *src = masks + ((size_t)img * G + g) * (size_t)H * W;
        const int len = x1 - x0, k = threadIdx.x & 15;
        if (len > 0)
            for (int y = y0 + (threadIdx.x >> 4); y < y1; y += TB / 16) {
                const unsigned char *s = src + (size_t)y * W + x0;
                int head = (int)((16 - (reinterpret_cast<uintptr_t>(s) & 15)) & 15);
                head = head < len ? head : len;
                const int nvec = (len - head) >> 4, tail0 = head + (nvec << 4);
                if (k < head) v[0] += s[k] != 0;
                if (tail0 + k < len) v[0] += s[tail0 + k] != 0;
                const uint4 *pv = reinterpret_cast<const uint4 *>(s + head);
                for (int i = k; i < nvec; i += 16) {
                    const uint4 q = pv[i];
                    v[0] += nz_bytes(q.x) + nz_bytes(q.y) + nz_bytes(q.z) + nz_bytes(q.w);
                }
            }
        const int HWm = msz * msz;
        const float *lg = mask_out + (size_t)r * HWm * Cp + ch;
        const int32_t *gm = gt_roi_mask + (size_t)r * HWm;
        for (int p = threadIdx.x; p < HWm; p += TB) {
            const int pr = lg[(size_t)p * Cp] > 0.f, gt = gm[p] > 0;
            v[1] += pr; v[2] += gt; v[3] += pr & gt;
        }
    }
    block_sum_i<4, TB>(v);
    if (threadIdx.x != 0) return;
    float t = 0.f;
    if (live && v[0] > 0 && full > 0) {
        const float full_est = ((float)v[2] * (float)full) / (float)v[0];
        const float uni = ((float)v[1] + full_est) - (float)v[3];
        t = (float)v[3] / fmaxf(uni, 1.0f);
    }
    target[r] = t;
    if (counts) {
        int32_t *o = counts + (size_t)r * 5;
        o[0] = full; o[1] = v[0]; o[2] = v[1]; o[3] = v[2]; o[4] = v[3];
    }
}

// The head's input (Rm, P, P, cin_p), one thread per float4: channels [0, C) the pooled features, channel C the 2x2/2 max of the class
// logit - fmaxf(fmaxf(fmaxf(m[2y][2x], m[2y][2x+1]), m[2y+1][2x]), m[2y+1][2x+1]) - or 0 for a row without a channel, the rest zeros.
__global__ __launch_bounds__(NT) void k_maskiou_input_fwd(const float *__restrict__ feat, const float *__restrict__ mask_out,
                                                          const int32_t *__restrict__ label, int label_base, size_t n4, int P, int C4,
                                                          int Cp, int n_channels, int cin4, float *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
        const int q = (int)(i % cin4);
        const size_t pix = i / cin4;
        float4 o = f4(0.f);
        if (q < C4) {
            o = ld4(feat + (pix * C4 + q) * 4);
        } else if (q == C4) {
            const int x = (int)(pix % P), y = (int)((pix / P) % P);
            const size_t r = pix / ((size_t)P * P);
            const int ch = label[r] - label_base;
            if (ch >= 0 && ch < n_channels) {
                const float *m = mask_out + ((r * 2 * P + 2 * y) * 2 * P + 2 * x) * Cp + ch;
                const size_t line = (size_t)2 * P * Cp;
                o.x = fmaxf(fmaxf(fmaxf(m[0], m[Cp]), m[line]), m[line + Cp]);
            }
        }
        st4(out + i * 4, o);
    }
}

// g_pool (Rm, P, P, C) += g_in (Rm, P, P, cin_p)[..., :C]: one add per element
__global__ __launch_bounds__(NT) void k_maskiou_input_bwd(const float *__restrict__ g_in, size_t n4, int C4, int cin4,
                                                          float *__restrict__ g_pool) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) {
        const size_t pix = i / C4;
        const int q = (int)(i % C4);
        const float4 a = ld4(g_pool + i * 4), b = ld4(g_in + (pix * cin4 + q) * 4);
        st4(g_pool + i * 4, make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w));
    }
}

// PHASE 0: (weight * sum of 0.5 d^2, count) over the rows with target > 0, d = pred[r, label - label_base] - target[r].
// PHASE 1: every element of gx (Rm, ld): d * (weight * (1 / count)) at that column of those rows, 0 elsewhere.
template <int PHASE>
__global__ __launch_bounds__(NT) void k_maskiou_l2(const float *__restrict__ pred, int ld, int n_channels, const float *__restrict__ target,
                                                   const int32_t *__restrict__ label, int label_base, int Rm, float weight,
                                                   float *__restrict__ part, const float *__restrict__ norm, float *__restrict__ gx) {
    if (PHASE == 0) {
        float ls = 0.f, cnt = 0.f;
        for (int r = blockIdx.x * NT + threadIdx.x; r < Rm; r += gridDim.x * NT) {
            const int ch = label[r] - label_base;
            const float t = target[r];
            if (!(t > 0.f) || ch < 0 || ch >= n_channels) continue;
            const float d = pred[(size_t)r * ld + ch] - t;
            ls += 0.5f * d * d;
            cnt += 1.f;
        }
        block_partial(ls * weight, cnt, part);
    } else {
        const float scale = weight * (1.0f / norm[1]);
        const size_t n = (size_t)Rm * ld;
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
            const int r = (int)(i / ld), c = (int)(i % ld), ch = label[r] - label_base;
            const float t = target[r];
            gx[i] = (t > 0.f && ch >= 0 && ch < n_channels && c == ch) ? (pred[i] - t) * scale : 0.f;
        }
    }
}

__global__ __launch_bounds__(NT) void k_maskiou_rescore(const float *__restrict__ score, const float *__restrict__ pred, int ld,
                                                        int n_channels, const int32_t *__restrict__ label, int D, float *__restrict__ out) {
    const int d = blockIdx.x * NT + threadIdx.x;
    if (d >= D) return;
    const int ch = label[d];
    const float iou = (ch >= 0 && ch < n_channels) ? pred[(size_t)d * ld + ch] : 0.f;
    out[d] = score[d] * fminf(fmaxf(iou, 0.f), 1.f);
}

int ew_blocks(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>((n + NT - 1) / NT, 65535)); }

}  // namespace

extern "C" size_t mrcnn_maskiou_target_workspace_bytes(int N, int G) {
    if (N <= 0 || G <= 0) return 0;
    return (size_t)N * G * MI_CHUNKS * sizeof(int32_t);
}

extern "C" int mrcnn_maskiou_target(const uint8_t *masks, int N, int G, int H, int W, const int32_t *n_gt, const float *sample_roi,
                                    const int32_t *gt_assign, const int32_t *label, const int32_t *n_pos, int n_sample, int rows,
                                    const float *mask_out, int mask_size, int Cp, int n_channels, const int32_t *gt_roi_mask,
                                    int label_base, int32_t *area, float *target, int32_t *counts, void *ws, size_t ws_bytes,
                                    void *stream) {
    if (N <= 0 || G <= 0 || H <= 0 || W <= 0 || n_sample <= 0 || rows < 0 || rows > n_sample || mask_size <= 0 || Cp <= 0 || N > 65535 ||
        G > 65535)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_target: bad sizes (N, G, H, W, n_sample, mask_size, Cp > 0; 0 <= rows <= n_sample)");
    if (n_channels <= 0 || n_channels > Cp)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_target: %d label channels outside the %d of mask_out", n_channels, Cp);
    if ((long long)N * rows > (1 << 30) || (long long)N * G > (1 << 24))
        return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "maskiou_target: too many rows or masks");
    if (rows == 0) return 0;
    if (!masks || !n_gt || !sample_roi || !gt_assign || !label || !n_pos || !mask_out || !gt_roi_mask || !area || !target || !ws)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_target: null pointer");
    if (ws_bytes < mrcnn_maskiou_target_workspace_bytes(N, G))
        return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "maskiou_target: workspace %zu < %zu", ws_bytes, mrcnn_maskiou_target_workspace_bytes(N, G));
    hipStream_t st = (hipStream_t)stream;
    int32_t *part = (int32_t *)ws;
    const int Rm = N * rows;
    hipLaunchKernelGGL(k_mask_area, dim3(MI_CHUNKS, G, N), dim3(NT), 0, st, masks, G, (long long)H * W, n_gt, part);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_maskiou_target, dim3(Rm + mrcnn::cdiv(N * G, TB)), dim3(TB), 0, st, masks, N, G, H, W, n_gt, part, area, sample_roi,
                       gt_assign, label, n_pos, n_sample, rows, Rm, mask_out, mask_size, Cp, n_channels, gt_roi_mask, label_base, target, counts);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_maskiou_input_fwd(const float *feat, const float *mask_out, const int32_t *label, int label_base, int Rm, int P,
                                       int C, int Cp, int n_channels, int cin_p, float *out, void *stream) {
    if (Rm < 0 || P <= 0 || C <= 0 || Cp <= 0 || cin_p <= 0 || (C % 4) || (cin_p % 4) || cin_p < C + 4)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_input_fwd: bad sizes (C and cin_p multiples of 4, cin_p >= C + 4)");
    if (n_channels <= 0 || n_channels > Cp)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_input_fwd: %d label channels outside the %d of mask_out", n_channels, Cp);
    if (Rm == 0) return 0;
    if (!feat || !mask_out || !label || !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_input_fwd: null pointer");
    const size_t n4 = (size_t)Rm * P * P * (cin_p / 4);
    hipLaunchKernelGGL(k_maskiou_input_fwd, dim3(ew_blocks(n4)), dim3(NT), 0, (hipStream_t)stream, feat, mask_out, label, label_base, n4, P,
                       C / 4, Cp, n_channels, cin_p / 4, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_maskiou_input_bwd(const float *g_in, int Rm, int P, int C, int cin_p, float *g_pool, void *stream) {
    if (Rm < 0 || P <= 0 || C <= 0 || cin_p <= 0 || (C % 4) || (cin_p % 4) || cin_p < C)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_input_bwd: bad sizes (C and cin_p multiples of 4, cin_p >= C)");
    if (Rm == 0) return 0;
    if (!g_in || !g_pool) return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_input_bwd: null pointer");
    const size_t n4 = (size_t)Rm * P * P * (C / 4);
    hipLaunchKernelGGL(k_maskiou_input_bwd, dim3(ew_blocks(n4)), dim3(NT), 0, (hipStream_t)stream, g_in, n4, C / 4, cin_p / 4, g_pool);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_maskiou_l2(const float *pred, int ld, int n_channels, const float *target, const int32_t *label, int label_base, int Rm,
                                float weight, float *loss_out, float *gx, void *ws, size_t ws_bytes, void *stream) {
    if (Rm < 0 || ld <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_l2: bad sizes");
    if (n_channels <= 0 || n_channels > ld)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_l2: %d label channels outside the %d columns of pred", n_channels, ld);
    if (!(weight > 0.f) || weight > 3.0e38f) return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_l2: weight must be a finite number above 0");
    if ((Rm > 0 && (!pred || !target || !label)) || !loss_out || !ws) return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_l2: null pointer");
    if (ws_bytes < mrcnn_loss_workspace_bytes()) return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "maskiou_l2: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)ws;
    const int nb = grid_for(Rm);
    hipLaunchKernelGGL(k_maskiou_l2<0>, dim3(nb), dim3(NT), 0, st, pred, ld, n_channels, target, label, label_base, Rm, weight, part, nullptr,
                       nullptr);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, st, part, nb, loss_out);
    MRCNN_LAUNCH_CHECK();
    if (gx && Rm > 0) {
        hipLaunchKernelGGL(k_maskiou_l2<1>, dim3(grid_for((long long)Rm * ld)), dim3(NT), 0, st, pred, ld, n_channels, target, label, label_base,
                           Rm, weight, part, loss_out, gx);
        MRCNN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mrcnn_maskiou_rescore(const float *score, const float *pred, int ld, int n_channels, const int32_t *label, int D, float *out,
                                     void *stream) {
    if (D < 0 || ld <= 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_rescore: bad sizes");
    if (n_channels <= 0 || n_channels > ld)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_rescore: %d label channels outside the %d columns of pred", n_channels, ld);
    if (D == 0) return 0;
    if (!score || !pred || !label || !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "maskiou_rescore: null pointer");
    hipLaunchKernelGGL(k_maskiou_rescore, dim3(mrcnn::cdiv(D, NT)), dim3(NT), 0, (hipStream_t)stream, score, pred, ld, n_channels, label, D, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
