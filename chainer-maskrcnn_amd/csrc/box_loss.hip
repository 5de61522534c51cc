// IoU-based box regression losses (GIoU, DIoU, CIoU) on the decoded box, forward + hand-derived gradient, for gfx950.
//
// An alternative to mrcnn_smooth_l1_f32 with the same inputs, the same normaliser and the same gradient-buffer contract: the predicted
// deltas and the encoded targets of a row are both decoded against the row's RoI / anchor with box_common.h's loc_denorm4, box_cs,
// loc2cs and cs_corners (d = v * std + mean, centre / size, expf, corners: the functions detect_decode_row, k_decode and
// k_cascade_refine call; no un-scaling, no clipping), and the loss is taken on the two boxes.  The IoU here carries BOX_EPS and
// derivatives: a rule of its own, not box_common.h's.  The gradient goes back through the IoU terms, the decode and std to the deltas.
//
// Latency-bound, not bandwidth-bound: almost every row of the RPN call (and three quarters of the head's) has label <= 0 and costs one
// label load and, in the gradient pass, one zero store.  The label is tested first; x, t and the RoI are loaded for positive rows only.
// Three launches like k_sl1: block partials, k_finalize (loss_common.h: fixed order, no float atomics), gradient.
#include "loss_common.h"
#include "box_common.h"

#pragma clang fp contract(off)

namespace {

constexpr float BOX_EPS = 1e-7f;
constexpr float BOX_DSIZE_MAX = 4.135166556742356f;     // log(1000 / 16): predicted dh, dw are clamped above before expf
constexpr float FOUR_OVER_PI2 = 0.4052847345693511f;    // 4 / pi^2

__device__ __forceinline__ float4 load_row4(const float *p, bool vec) {
    return vec ? ld4(p) : make_float4(p[0], p[1], p[2], p[3]);
}

// The share of a max(a, b) - or of a min(b, a) - that belongs to a: all of it where a is the larger, half at a tie (so that identical
// boxes, the minimum of every loss here, get no push from the kinks), none otherwise.
__device__ __forceinline__ float tie_weight(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }

// One axis of the two boxes, the prediction as (centre pc, size ps) and the target as corners (g1, g2): the overlap i = max(0, min of the
// far sides - max of the near sides), the side c of the enclosing box, and their derivatives by pc (_c) and ps (_s).  A tie of a
// min / max splits the derivative evenly; the clamp at 0 passes it where the overlap is positive.
struct Axis { float i, c, i_c, i_s, c_c, c_s; };
template <bool GRAD>
__device__ __forceinline__ Axis axis_terms(float p1, float p2, float g1, float g2) {
    Axis a;
    const float raw = fminf(p2, g2) - fmaxf(p1, g1);
    a.i = fmaxf(raw, 0.f);
    a.c = fmaxf(p2, g2) - fminf(p1, g1);
    if (GRAD) {
        const float on = raw > 0.f ? 1.f : 0.f;
        const float i1 = on * tie_weight(p1, g1), i2 = on * tie_weight(g2, p2);       // d i = i2 d p2 - i1 d p1: the inner sides
        const float c1 = tie_weight(g1, p1), c2 = tie_weight(p2, g2);                 // d c = c2 d p2 - c1 d p1: the outer sides
        a.i_c = i2 - i1; a.i_s = 0.5f * (i2 + i1);                                    // p1 = pc - ps / 2, p2 = pc + ps / 2
        a.c_c = c2 - c1; a.c_s = 0.5f * (c2 + c1);
    } else {
        a.i_c = a.i_s = a.c_c = a.c_s = 0.f;
    }
    return a;
}

// The loss of one row; GRAD: g[0..4) = d L / d x (without weight and normaliser).
template <bool GRAD>
__device__ __forceinline__ float box_loss_row(float4 xv, float4 tv, float4 roi, int kind, float4 mean, float4 stdv, float *g) {
    const float4 rc = box_cs(roi), dp = loc_denorm4(xv, stdv, mean);
    const float h = rc.z, w = rc.w, dh = dp.z, dw = dp.w;
    // prediction: centre (pcy, pcx), size (ph, pw); dh, dw clamped above before the decode
    const float pcy = loc2centre1(dp.x, h, rc.x), pcx = loc2centre1(dp.y, w, rc.y);
    const float ph = loc2size1(fminf(dh, BOX_DSIZE_MAX), h), pw = loc2size1(fminf(dw, BOX_DSIZE_MAX), w);
    const float4 pb = cs_corners(make_float4(pcy, pcx, ph, pw));
    // target (not clamped)
    const float4 gc = loc2cs(rc, loc_denorm4(tv, stdv, mean));
    const float gcy = gc.x, gcx = gc.y, gh = gc.z, gw = gc.w;
    const float4 gb = cs_corners(gc);

    const Axis ay = axis_terms<GRAD>(pb.x, pb.z, gb.x, gb.z), ax = axis_terms<GRAD>(pb.y, pb.w, gb.y, gb.w);
    const float inter = ay.i * ax.i;
    const float uni = ((ph * pw + gh * gw) - inter) + BOX_EPS;
    const float iou = inter / uni;
    float L = 1.0f - iou;
    // d L by (pcy, ph, pcx, pw)
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (GRAD) {
        const float di[4] = {ay.i_c * ax.i, ay.i_s * ax.i, ay.i * ax.i_c, ay.i * ax.i_s};     // d inter
        const float da[4] = {0.f, pw, 0.f, ph};                                                // d (area of the prediction)
        const float u2 = uni * uni;
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = -((di[k] * (uni + inter) - inter * da[k]) / u2);   // d union = da - di
        if (kind == MRCNN_BOX_LOSS_GIOU) {
            const float ce = ay.c * ax.c + BOX_EPS;
            const float dc[4] = {ay.c_c * ax.c, ay.c_s * ax.c, ay.c * ax.c_c, ay.c * ax.c_s};
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] += dc[k] * (uni + BOX_EPS) / (ce * ce) - (da[k] - di[k]) / ce;
        }
    }
    if (kind == MRCNN_BOX_LOSS_GIOU) {
        const float c = ay.c * ax.c;
        L += (c - uni) / (c + BOX_EPS);
    } else {
        const float ry = pcy - gcy, rx = pcx - gcx;
        const float rho2 = ry * ry + rx * rx;
        const float dd = (ay.c * ay.c + ax.c * ax.c) + BOX_EPS;
        L += rho2 / dd;
        if (GRAD) {
            const float q = rho2 / (dd * dd);
            d[0] += 2.0f * ry / dd - q * (2.0f * ay.c * ay.c_c);
            d[1] += -q * (2.0f * ay.c * ay.c_s);
            d[2] += 2.0f * rx / dd - q * (2.0f * ax.c * ax.c_c);
            d[3] += -q * (2.0f * ax.c * ax.c_s);
        }
        if (kind == MRCNN_BOX_LOSS_CIOU) {
            const float hpe = ph + BOX_EPS;
            const float da_ = atanf(gw / (gh + BOX_EPS)) - atanf(pw / hpe);
            const float v = FOUR_OVER_PI2 * (da_ * da_);
            const float alpha = v / (((1.0f - iou) + v) + BOX_EPS);       // a constant in the gradient
            L += alpha * v;
            if (GRAD) {
                const float den = hpe * hpe + pw * pw;
                const float s = alpha * (2.0f * FOUR_OVER_PI2) * da_;     // - alpha * d v / d atan(pw / hpe)
                d[1] += s * (pw / den);                                   // d atan / d ph = -pw / den
                d[3] += -s * (hpe / den);                                 // d atan / d pw = hpe / den
            }
        }
    }
    if (GRAD) {
        g[0] = d[0] * h * stdv.x;
        g[1] = d[2] * w * stdv.y;
        g[2] = dh <= BOX_DSIZE_MAX ? d[1] * ph * stdv.z : 0.f;            // a clamped coordinate has gradient exactly 0
        g[3] = dw <= BOX_DSIZE_MAX ? d[3] * pw * stdv.w : 0.f;
    }
    return L;
}

// vx / vtr / vg: x rows, (t and rois) rows, gx rows (and its fill) are 16-byte aligned and are moved as float4
template <int PHASE>   // 0: loss partials, 1: gradient
__global__ __launch_bounds__(NT) void k_box_iou(const float *__restrict__ x, int ldx, const float *__restrict__ t,
                                                const float *__restrict__ rois, int roi_period, const int32_t *__restrict__ label,
                                                int M, int kind, float4 mean, float4 stdv, float weight, int vx, int vtr, int vg,
                                                float *__restrict__ part, const float *__restrict__ norm, float *__restrict__ gx,
                                                int ldg, int gfill) {
    float ls = 0.f, cnt = 0.f;
    const float scale = PHASE ? weight * (1.0f / norm[1]) : 0.f;
    for (long long r = (long long)blockIdx.x * NT + threadIdx.x; r < M; r += (long long)gridDim.x * NT) {
        const int lb = label[r];
        if (PHASE == 0 && lb >= 0) cnt += 1.f;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (lb > 0) {
            const float4 xv = load_row4(x + (size_t)r * ldx, vx), tv = load_row4(t + (size_t)r * 4, vtr);
            const float4 roi = load_row4(rois + (size_t)(r % roi_period) * 4, vtr);
            const float L = box_loss_row<PHASE == 1>(xv, tv, roi, kind, mean, stdv, g);
            if (PHASE == 0) ls += L;
        }
        if (PHASE == 1) {
            float *o = gx + (size_t)r * ldg;
            const float4 gv = make_float4(g[0] * scale, g[1] * scale, g[2] * scale, g[3] * scale);
            int j = 4;
            if (vg) {
                st4(o, gv);
                for (; j + 4 <= gfill; j += 4) st4(o + j, f4(0.f));
            } else {
                o[0] = gv.x; o[1] = gv.y; o[2] = gv.z; o[3] = gv.w;
            }
            for (; j < gfill; ++j) o[j] = 0.f;
        }
    }
    if (PHASE == 0) block_partial(ls * weight, cnt, part);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// x (M, ldx >= 4) predicted deltas, t (M,4) encoded targets, rois (roi_period,4) (y1,x1,y2,x2): row r is relative to rois[r % roi_period];
// label (M,): rows with label > 0 carry loss, the normaliser is #(label >= 0).  mean4 / std4: HOST arrays, read during the call.
extern "C" int mrcnn_box_iou_loss_f32(const float *x, int ldx, const float *t, const float *rois, int roi_period, const int32_t *label,
                                      int M, int kind, const float *mean4, const float *std4, float weight, float *loss_out, float *gx,
                                      int ldg, int gfill, void *ws, size_t ws_bytes, void *stream) {
    if ((M > 0 && (!x || !t || !rois || !label)) || !loss_out || !ws || !mean4 || !std4 || M < 0 || ldx < 4 || roi_period <= 0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "box_iou_loss: bad arguments (null pointer, M < 0, ldx < 4 or roi_period <= 0)");
    if (kind != MRCNN_BOX_LOSS_GIOU && kind != MRCNN_BOX_LOSS_DIOU && kind != MRCNN_BOX_LOSS_CIOU)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "box_iou_loss: kind %d is none of MRCNN_BOX_LOSS_GIOU, _DIOU, _CIOU", kind);
    if (gx && (gfill < 0 || ldg < std::max(4, gfill)))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "box_iou_loss: ldg %d is below max(4, gfill = %d)", ldg, gfill);
    if (ws_bytes < mrcnn_loss_workspace_bytes()) return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "box_iou_loss: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)ws;
    const int nb = grid_for(M);
    const float4 mean = make_float4(mean4[0], mean4[1], mean4[2], mean4[3]), stdv = make_float4(std4[0], std4[1], std4[2], std4[3]);
    const int vx = (ldx % 4 == 0 && aligned16(x)) ? 1 : 0, vtr = (aligned16(t) && aligned16(rois)) ? 1 : 0;
    const int vg = (gx && ldg % 4 == 0 && aligned16(gx)) ? 1 : 0;
    hipLaunchKernelGGL(k_box_iou<0>, dim3(nb), dim3(NT), 0, st, x, ldx, t, rois, roi_period, label, M, kind, mean, stdv, weight, vx, vtr,
                       vg, part, nullptr, nullptr, 0, 0);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, st, part, nb, loss_out);
    MRCNN_LAUNCH_CHECK();
    if (gx && M > 0) {
        hipLaunchKernelGGL(k_box_iou<1>, dim3(nb), dim3(NT), 0, st, x, ldx, t, rois, roi_period, label, M, kind, mean, stdv, weight, vx,
                           vtr, vg, part, loss_out, gx, ldg, gfill);
        MRCNN_LAUNCH_CHECK();
    }
    return 0;
}
