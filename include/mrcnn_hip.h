/*
 * mrcnn_hip.h - C ABI of libmrcnn_hip.so: the MI355X (gfx950) kernels of the FPN Mask R-CNN
 * training path of katotetsuro/chainer-maskrcnn.
 *
 * The reference is pure Python on Chainer/CuPy and has no FFI of its own; every entry point
 * below names the reference interface (file:line under the reference tree) whose device work
 * it replaces.  The binding a reference maintainer would add is a ctypes stub - see
 * INTEGRATION.md.  The in-repo host layer (chainer-maskrcnn_amd/chainer_maskrcnn/_hip) is
 * exactly such a stub over torch tensors.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless marked "host".
 *   - the caller owns every buffer, including workspaces (query *_workspace_bytes first);
 *     the library never allocates or frees device memory and keeps no pointer past return.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream); no call synchronises the device - with ONE exception, the explicit status query
 *     mrcnn_roi_align_bwd_plan_status (ABI v9).  The composite calls (mrcnn_bottleneck_*) also enqueue on the
 *     caller's side stream, behind events of a small library-owned pool (no device memory).
 *   - return value: 0 = success; negative = MRCNN_E_* argument error; positive = hipError_t.
 *     mrcnn_last_error() returns a thread-local message for the last failure.
 *   - no C++ exceptions cross this boundary.
 *   - layouts: MRCNN_LAYOUT_NCHW is the reference's (Chainer) layout; MRCNN_LAYOUT_NHWC
 *     (channel innermost) is the layout the fast kernels are written for.  A torch tensor
 *     of logical shape (N,C,H,W) in torch.channels_last memory format IS MRCNN_LAYOUT_NHWC.
 */
#ifndef MRCNN_HIP_H
#define MRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRCNN_ABI_VERSION 10

enum {
    MRCNN_OK = 0,
    MRCNN_E_INVALID = -1,      /* bad argument (null pointer, non-positive size, ...) */
    MRCNN_E_UNSUPPORTED = -2,  /* valid but not implemented for this shape/layout */
    MRCNN_E_WORKSPACE = -3     /* workspace too small */
};

enum { MRCNN_LAYOUT_NCHW = 0, MRCNN_LAYOUT_NHWC = 1 };

#define MRCNN_MAX_LEVELS 8

int mrcnn_abi_version(void);
const char *mrcnn_last_error(void);

/* ------------------------------------------------------------------------------------------
 * ROIAlign.  Replaces chainer_maskrcnn.functions.roi_align.roi_align_2d.roi_align_2d(x, rois,
 * outh, outw, spatial_scale) -- the un-vendored submodule called through
 * chainer_maskrcnn/functions/roi_align_2d_yx.py:4-7 -- and its autograd backward.
 *
 *   x     (N,C,H,W) f32 in `layout`
 *   rois  (R,5) f32 rows (batch_idx, x1, y1, x2, y2) in image pixels (already xy order,
 *         i.e. AFTER the [0,2,1,4,3] permutation of roi_align_2d_yx.py:5)
 *   y     (R,C,PH,PW) f32 in `layout` (NHWC => (R,PH,PW,C))
 *   sampling_ratio  >0: fixed grid per bin; 0: adaptive ceil(roi_size/pooled_size)
 * Algorithm: Caffe2/Detectron RoIAlign (legacy, non-aligned), float32, no FMA contraction in
 * the coordinate arithmetic - identical, operation for operation, to oracle/roi_align.py.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_roi_align_fwd_f32(const float *x, int layout, int N, int C, int H, int W,
                            const float *rois, int R, int PH, int PW, float spatial_scale,
                            int sampling_ratio, float *y, void *stream);
/* The same call with the caller's scratch of mrcnn_roi_align_fwd_workspace_bytes(R) bytes (ABI v6).  With it the NHWC fast path
 * walks the RoIs in MAP ORDER: a first small kernel ranks them by (level, image, 64-row band of the box centre, centre column)
 * and the forward kernel processes RoI perm[i] at position i, writing ITS output rows - the reference's per-RoI loop
 * (fpn_roi_mask_head.py:59-61) has no order dependence, the results are the same bits in the same rows, and co-resident waves
 * read neighbouring map lines instead of random ones.  Without scratch (or R < 128, or R > 8192): caller order. */
int mrcnn_roi_align_fwd_ws_f32(const float *x, int layout, int N, int C, int H, int W,
                               const float *rois, int R, int PH, int PW, float spatial_scale,
                               int sampling_ratio, float *y, void *ws, size_t ws_bytes, void *stream);
size_t mrcnn_roi_align_fwd_workspace_bytes(int R);
/* A/B switch of the map-order walk (process-wide; default 1 = on when scratch is given). */
int mrcnn_roi_align_set_fwd_map_order(int on);

/* Backward (adjoint scatter).  gx is fully overwritten (callee zero-fills cells no RoI touches).
 * Fast path (NHWC, C%4==0, PH,PW<=16, sampling_ratio>0): owner-computes tiles, no atomics,
 * bit-reproducible.  Other shapes: memset + atomic scatter.
 * mrcnn_roi_align_bwd_ws_f32 takes the caller's scratch of mrcnn_roi_align_bwd_workspace_bytes() bytes (the RoI-split slabs of small
 * maps); mrcnn_roi_align_bwd_f32 = the same call without scratch.  Both give identical bits. */
int mrcnn_roi_align_bwd_f32(const float *gy, int layout, int N, int C, int H, int W,
                            const float *rois, int R, int PH, int PW, float spatial_scale,
                            int sampling_ratio, float *gx, void *stream);
int mrcnn_roi_align_bwd_ws_f32(const float *gy, int layout, int N, int C, int H, int W,
                               const float *rois, int R, int PH, int PW, float spatial_scale,
                               int sampling_ratio, float *gx, void *ws, size_t ws_bytes, void *stream);
size_t mrcnn_roi_align_bwd_workspace_bytes(int N, int C, int H, int W, int R, int PH, int PW, int sampling_ratio);

/* Multi-level (FPN) batched variants: ONE launch for all RoIs over all pyramid levels.
 * Replace the per-RoI Python loops of chainer_maskrcnn/model/head/fpn_roi_mask_head.py:59-61,
 * 75-77,93-94 (and fpn_roi_keypoint_head.py:63-68,85-86,102-103).
 *   xs / gxs        host arrays of L device base pointers (level l: (N,C,Hs[l],Ws[l]) NHWC)
 *   Hs, Ws, scales  host arrays of length L  (scales[l] = spatial_scales[l])
 *   levels          (R,) int32 device, level of each RoI (already clipped to [0,L))
 *   rois            (R,5) f32 device (batch_idx,x1,y1,x2,y2)
 *   y / gy          (R,PH,PW,C) f32
 *   accumulate      backward: 0 = every gxs[l] is overwritten (zero where no RoI lands),
 *                   1 = gradients are added to gxs[l] (second pooled size over the same pyramid)
 *   ws, ws_bytes    backward: optional device scratch of mrcnn_roi_align_fpn_bwd_workspace_bytes() bytes
 *                   ([slabs][per-RoI tables of variant 3]).  With it, levels with few 8x8 tiles (the coarse ones, where map_rois_to_fpn_levels puts most RoIs) are
 *                   computed by several workgroups per tile over disjoint RoI subsets and summed in fixed order;
 *                   without it (NULL) one workgroup per tile does all the RoIs.  Results are bit-reproducible
 *                   either way (the two modes differ from each other by summation order only).
 * Only MRCNN_LAYOUT_NHWC with C%4==0 is supported. */
int mrcnn_roi_align_fpn_fwd_f32(const float *const *xs, const int *Hs, const int *Ws,
                                const float *scales, int L, int N, int C, const float *rois,
                                const int32_t *levels, int R, int PH, int PW,
                                int sampling_ratio, float *y, void *stream);
/* forward with scratch of mrcnn_roi_align_fwd_workspace_bytes(R) bytes: map-order walk, see mrcnn_roi_align_fwd_ws_f32 */
int mrcnn_roi_align_fpn_fwd_ws_f32(const float *const *xs, const int *Hs, const int *Ws,
                                   const float *scales, int L, int N, int C, const float *rois,
                                   const int32_t *levels, int R, int PH, int PW,
                                   int sampling_ratio, float *y, void *ws, size_t ws_bytes, void *stream);
int mrcnn_roi_align_fpn_bwd_f32(const float *gy, float *const *gxs, const int *Hs, const int *Ws,
                                const float *scales, int L, int N, int C, const float *rois,
                                const int32_t *levels, int R, int PH, int PW,
                                int sampling_ratio, int accumulate, void *ws, size_t ws_bytes, void *stream);
size_t mrcnn_roi_align_fpn_bwd_workspace_bytes(const int *Hs, const int *Ws, int L, int N, int C, int R, int PH, int PW,
                                               int sampling_ratio);
/* (ABI v9) The backward in two launches.  Which (RoI, bin) pairs land on which 4 x 4 patch of the gradient map - two thirds of a wave's
 * life in the fused backward - depends on the RoIs only, and in a training step the RoIs are known a whole head before the backward
 * (the reference runs the forward with them: fpn_roi_mask_head.py:59-61,75-77).  mrcnn_roi_align_fpn_bwd_plan_f32 writes every patch's
 * entry list ((gy row, 4 row weights, 4 column weights), in (RoI, ph, pw) order) into the caller's `plan` buffer of
 * mrcnn_roi_align_fpn_bwd_plan_bytes() bytes - on any stream, any time after the RoIs exist; mrcnn_roi_align_fpn_bwd_planned_f32 is
 * mrcnn_roi_align_fpn_bwd_f32 that streams gy along those lists: same entry order, same weights, same FMAs = the same bits FOR FINITE gy
 * (the lean kernel multiplies every row of a patch by its weight, zero weights included, where the fused kernel skips a zero-weight row: an
 * Inf / NaN in gy reaches all 16 cells of the patches it touches instead of the rows it lands on - still non-finite output, other cells).
 * The plan is checked on the device (magic, level count and every level's H x W, N, RoI count, pooled size, sampling ratio, node capacity
 * against this call's plan_bytes; a tile whose entries did not fit the pool is flagged): what the plan does not hold is computed by the
 * fused kernel in a second launch.
 * The buffer must not be modified between the two calls, and both must see the same rois / levels / scales; split_levels != 0 iff the
 * backward call is given its mrcnn_roi_align_fpn_bwd_workspace_bytes() scratch (the coarse levels' RoI split).  L == 1 with
 * levels == NULL is the single-level form (configs[1]). */
size_t mrcnn_roi_align_fpn_bwd_plan_bytes(const int *Hs, const int *Ws, int L, int N, int R, int PH, int PW, int split_levels);
int mrcnn_roi_align_fpn_bwd_plan_f32(const int *Hs, const int *Ws, const float *scales, int L, int N, int C, const float *rois,
                                     const int32_t *levels, int R, int PH, int PW, int sampling_ratio, int split_levels,
                                     void *plan, size_t plan_bytes, void *stream);
/* measurement knob of the lean backward: gy rows in flight per wave / waves per SIMD / threads per workgroup: 0 = 10 / 8 / 512, 1 = 16 / 7 / 512,
 * 2 = 8 / 8 / 512 (a workgroup = one 8 x 8 tile), 8 = 8 / 8 / 256 (half a tile: the default), 9 = 8 / 8 / 128 (one patch); + 256 x bits
 * (1: no gy loads, 2: no gx stores - wrong results; 16: plain instead of non-temporal stores) */
int mrcnn_debug_roi_align_lean_variant(int v);
/* measurement: device buffer of 10 x u64 per wave (8 waves per 8 x 8 tile, tile-major) that the lean backward of the next planned calls fills -
 * s_memtime at entry / first node's loads back / end of the entry loop / stores acknowledged, entries, HW_ID | XCC_ID << 32, s_memrealtime
 * at entry / at the end, s_memtime when the kernel arguments / the node's scalar loads are back; null = off */
int mrcnn_debug_roi_align_lean_stamps(unsigned long long *stamps);
int mrcnn_roi_align_fpn_bwd_planned_f32(const float *gy, float *const *gxs, const int *Hs, const int *Ws, const float *scales, int L,
                                        int N, int C, const float *rois, const int32_t *levels, int R, int PH, int PW,
                                        int sampling_ratio, int accumulate, void *ws, size_t ws_bytes, void *plan,
                                        size_t plan_bytes, int plan_verified, void *stream);
/* plan_verified != 0: the caller has read mrcnn_roi_align_bwd_plan_status() for this plan after the builder finished and found
 * status3[0] == 1 (the builder's header) and status3[1] == 0 (no tile flagged): the call is then the lean kernel alone.  With 0 a second
 * launch follows it that computes the tiles the plan could not hold with the fused kernel - normally none, every workgroup leaves at
 * once, but their dispatch costs 3.5 - 5 us.  A training step passes 0 (it cannot afford the status query's synchronisation and does not
 * feel 5 us); the configs[1] microbenchmark verifies once, outside the timed region, and reports both.  status3 (host, 3 ints): header
 * valid, tiles flagged, pool nodes used.  mrcnn_roi_align_bwd_plan_status is the one entry point that WAITS for the device. */
int mrcnn_roi_align_bwd_plan_status(const void *plan, size_t plan_bytes, int *status3, void *stream);

/* Process-wide choice of the fast backward kernel: 2 (default) = one independent wave per 4x4 cell patch that derives the
 * geometry itself; 1 = the barrier-synchronised 8x8 tile kernel of round 1 (what tensors >= 4 GiB fall back to; selectable so
 * that tests reach it on small inputs).  Same results contract.  (ABI v10: the table-driven variant 3 and the forward-built
 * work plan of ABI v8 - mrcnn_roi_align_plan_workspace_bytes, mrcnn_roi_align_set_bwd_plan - are gone: both were measured
 * slower for the forward + backward pair and never shipped.) */
int mrcnn_roi_align_set_bwd_variant(int variant);

/* Diagnostic build of the backward kernel with s_memtime stamps at the phase boundaries of every wave (measurement
 * only).  stamps: 12 x u64 per wave, (8 * ceil(tiles / 8)) workgroups x 4 waves. */
int mrcnn_debug_roi_align_bwd_stamps(const float *gy, int N, int C, int H, int W, const float *rois, int R, int PH, int PW,
                                     float spatial_scale, int sampling_ratio, float *gx, unsigned long long *stamps,
                                     void *stream);

/* Measurement: block -> (XCD, CU) placement of a launch shaped like the ROIAlign backward (256 threads per block, all blocks co-resident
 * for spin_us): out[b] = HW_ID | XCC_ID << 32, out[nblocks + b] = s_memrealtime at the start of block b. */
int mrcnn_debug_dispatch_census(unsigned long long *out, int nblocks, int spin_us, void *stream);

/* Verification hook for the "ROIAlign indices bit-exact" contract: dumps, for every RoI and
 * both axes, the integer corner cells and float weights of every sample exactly as the
 * kernels compute them (same __device__ function).  Shapes as oracle.roi_align.
 * roi_align_sample_tables: cnt (R,2) i32, idx (R,2,smax,2) i32, wgt (R,2,smax,2) f32. */
int mrcnn_roi_align_sample_tables(const float *rois, int R, int H, int W, int PH, int PW,
                                  float spatial_scale, int sampling_ratio, int smax,
                                  int32_t *cnt, int32_t *idx, float *wgt, void *stream);

/* ------------------------------------------------------------------------------------------
 * Convolution (fp32 MFMA implicit GEMM).  Replaces the cuDNN/cuBLAS calls Chainer issues for
 * L.Convolution2D / L.Linear / L.Deconvolution2D in
 *   chainer_maskrcnn/model/extractor/feature_pyramid_network.py:22-40,48-68
 *   chainer_maskrcnn/model/rpn/multilevel_region_proposal_network.py:80-86,131-141
 *   chainer_maskrcnn/model/head/fpn_roi_mask_head.py:24-49,65-83
 * and their autograd backward passes.
 *   x  (N,H,W,Cin) NHWC      w  (Cout,KH,KW,Cin)      y  (N,Ho,Wo,Cout) NHWC
 *   Ho = (H + 2*pad - KH)/stride + 1.   Cout must be a multiple of 32 and Cin a multiple of 32 or
 *   exactly 4 (the image layer: K axis = (tap, 4 channels)); the host layer zero-pads channel
 *   counts such as 3, 18, 80, 81.  bias (Cout) may be NULL; relu != 0
 *   fuses max(.,0) into the forward epilogue.  Linear layers are 1x1 convolutions with
 *   H = W = 1; the 2x2/2 deconvolution is a 1x1 convolution to 4*Cout channels + a host view.
 * fwd / bwd_data take an optional workspace (mrcnn_conv2d_workspace_bytes; may be NULL/0): deep layers with few
 * pixels and a long K axis are split over K into slabs summed in fixed order (deterministic), so all CUs work.
 * bwd_data supports stride 1 only (a strided 1x1 convolution is a stride-1 one on the subsampled
 * lattice followed by mrcnn_subsample_bwd_f32); accumulate != 0 adds into gx instead of overwriting.  bwd_filter accumulates over pixels with a deterministic
 * split-K (slabs in the caller's workspace, fixed summation order); gbias may be NULL; accumulate != 0
 * adds into gw / gbias (layers shared by several inputs, e.g. the RPN head over 5 pyramid levels).
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_conv2d_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
/* Multiply-accumulates the MFMA pipes execute for ONE pass (forward, backward-data or backward-filter) of this layer:
 * N*Ho*Wo*KH*KW*Cin*Cout for the direct kernels, (m+2)^2 * tiles * Cin * Cout (2.25x / 4x fewer) where the 3x3 /
 * stride 1 / pad 1 layer takes the Winograd F(m x m,3x3) path (>= 256 channels, >= 2048 pixels) in that pass (pass: 0 forward,
 * 1 backward-data, 2 backward-filter).  For roofline accounting. */
long long mrcnn_conv2d_executed_macs(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int pass);
/* Process-wide selection of the Winograd path: thresholds (defaults 256 channels, 2048 pixels: measured break-even on
 * gfx950) and output tile (0 = per layer, whichever of F(2x2,3x3) / F(4x4,3x3) needs fewer multiplications; 2 or 4 =
 * forced).  Lowering the thresholds is how the tests run whole small networks through the Winograd kernels. */
int mrcnn_conv2d_set_winograd_thresholds(int min_channels, int min_pixels, int tile);
/* Per-pass override of the Winograd tile (forward, backward-data, backward-filter): 0 = follow the global tile above,
 * 2 / 4 = forced, -1 = that pass never takes the Winograd path.  Default (2, 0, 0): F(4x4,3x3) amplifies float32 rounding
 * far more than F(2x2,3x3).  In the forward pass of the ResNet conv2 layers that shows up as parameter-gradient errors of
 * up to 2e-2 (300x the float32 noise floor) in the layers fed by c4 / c5; in the backward passes, and in the forward pass of
 * the layers behind the backbone, it does not (profiles/r02_winograd_pass_probe.txt, r02_winograd_layer_probe.txt) - the
 * host layer therefore brackets the calls of its FPN / RPN / head convolutions with (0, ., .) (nn/core.py: Conv(fwd_tile=0)).
 * (0, 0, 0) = F(4x4) wherever it is cheaper in every pass of every layer: activations still within 2.2e-4 of their scale.
 * The setting is read on the host when a convolution entry point is called.  The getter writes the three current values. */
int mrcnn_conv2d_set_winograd_pass_tiles(int fwd, int bwd_data, int bwd_filter);
int mrcnn_conv2d_get_winograd_pass_tiles(int *tiles3);
/* EXPLORATORY, opt-in, never the default (and never bench.py's `value`): the forward-kind GEMM launches (forward convolutions and
 * both Winograd batched GEMMs) of a pass (forward, backward-data, backward-filter) with three-term split operands on the 16-bit
 * MFMA - every float32 operand staged as hi + lo planes, float32 accumulation of al*bh + ah*bl + ah*bh: 0 = float32 MFMA,
 * 1 = bf16 planes (16 significant bits, float32 range; ~4e-6 per product), 2 = IEEE-half planes (22 bits, ~5e-7 per product;
 * operands must stay below 65504 and lose relative precision below 6e-5), 3 = THREE bf16 planes hi + mid + lo (= the float32
 * operand exactly) and the six products of weight >= 2^-16 - a float32-ACCURATE emulation (the dropped terms are <= 3 x 2^-24 of
 * |ab|, the size of the float32 MFMA's own accumulation rounding) at 3/8 of the float32 MFMA cycles.  gfx950 has no xf32: this is
 * what challenging the 157.3 TF/s fp32-MFMA ceiling costs in accuracy and buys in time.  Values outside 0..3: MRCNN_E_ARG. */
int mrcnn_conv2d_set_split_operands(int fwd, int bwd_data, int bwd_filter);
/* The three modes in force (forward, backward-data, backward-filter), for callers that bracket a call with their own setting. */
int mrcnn_conv2d_get_split_operands(int *modes3);
/* Read-only plan query (tests, measurement): what the entry point of `pass` (0 forward, 1 backward-data, 2 backward-filter) would launch for
 * this geometry under the settings in force, given the workspace its size query asks for.  Computed by the dispatcher's own functions;
 * launches nothing, changes no setting.  Writes MRCNN_CONV_PLAN_FIELDS ints to out (n_out >= that):
 *   [0] path        0 un-split direct, 1 split-K, 2 tail split, 3 Winograd
 *   [1] bm, [2] bn  tile of the GEMM launch (256 x 256: the persistent plane GEMM)
 *   [3] ksplit      split count over K of that launch (backward-filter: the filter plan's)
 *   [4] tail_ks     tail-split factor (0 = none)
 *   [5] wino_m      0, 2 or 4
 *   [6] smallc      1 for the 4-channel image layer
 *   [7] arithmetic  the operand mode the launch really uses: 0 for the image layer whatever is set, else the pass's split mode
 *   [8] plane_gemm  1 when the batched Winograd GEMM goes to the persistent plane-GEMM kernels
 * Geometries the entry point declines (backward-data with stride > 1 or on the image layer, unpadded channels) return its error code. */
#define MRCNN_CONV_PLAN_FIELDS 9
int mrcnn_conv2d_plan_query(int pass, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int *out, int n_out);
/* Measurement knob (tools/gemm_only_profile.py): workgroups per CU the tile choice and the forward / backward-data split-K plan aim
 * for (default 2), the HALF rounds of workgroup slots the filter-gradient split-K fills (default 2 = one round), and a forced forward /
 * backward-data tile (0 = the planner's choice, 1 = 128x64, 2 = 64x64). */
int mrcnn_debug_conv_plan(int fill, int filter_rounds, int force_tile);
/* Measurement knob, tile order of the Winograd input transforms (speed only, same results): 0 = launch order, 1 = XCD-banded raster order,
 * n >= 2 = XCD-banded column panels n tiles wide (default 16). */
int mrcnn_debug_wino_banded(int on);
/* Measurement knob, split-operand GEMM kernels only: 1 = the MFMAs are skipped, 2 = the global loads inside the K loop are skipped,
 * 4 = the epilogue is skipped (results are garbage while one of these bits is set; where does such a kernel's time go?);
 * 8 = the three-plane (bf16x6) kernels run the plain K loop (split + LDS stores between the barriers) instead of the pipelined one
 * (split in registers in the MFMAs' shadow, loads two steps ahead) - same results, for A/B.  Bits 1 and 2 act on the plain loop. */
int mrcnn_debug_conv_parts(int mask);
/* Test / measurement entry points of the plane GEMMs (csrc/planes_gemm.h), the kernels behind split mode 3 on the Winograd path.
 * split_planes: float32 (R, C), C % 16 == 0 -> "P16" planes, unsigned short [R][C/16][3][16]: hi, mid, lo bf16 planes of 16
 * consecutive channels in 96 contiguous bytes (hi + mid + lo == x exactly).
 * planes_gemm, kind 0 (F): c (M, N) = sum_k a[m][k] b[batch(m)][n][k] - a = P16 (M, K), b = P16 (nbatch * N, K), batch(m) =
 * m / batch_rows, M = nbatch * batch_rows, batch_rows % 128 == 0; tile bm x bn = 128 x 128 | 64.
 * kind 1 (G): c (ksplit, M, nbatch, N) partial sums over the row ranges of a = P16 (nbatch * K, M), b = P16 (nbatch * K, N),
 * K = batch_rows, K % (16 * ksplit) == 0; tiles 128 | 64 each way.  Six v_mfma_f32_32x32x16_bf16 per product, float32 accumulate. */
int mrcnn_debug_split_planes_f32(const float *x, void *planes, int R, int C, int r4, void *stream);
int mrcnn_debug_planes_gemm_stamps(unsigned long long *stamps);
int mrcnn_debug_planes_gemm(int kind, const void *a, const void *b, float *c, int M, int N, int K, int batch_rows, int nbatch,
                            int ksplit, int bm, int bn, void *stream);

/* Measurement knob for bench.py's roofline split (never set on a product path): bit 0 skips the MFMA GEMM launches of
 * the convolution calls, bit 1 skips every other kernel they launch (Winograd transforms, slab / tail / column sums),
 * bit 2 makes the filter-gradient call return at once, bit 3 skips only that call's split-K slab sums (tools/ab_step.py:
 * what the weight-gradient stream costs the step).  Outputs are garbage while a bit is set; 0 restores normal operation. */
int mrcnn_conv2d_set_debug_skip(int mask);
/* The same kind of knob for the BatchNorm calls: bit 0 leaves out the backward's finalisation launch, bit 1 the forward's (the form fed by
 * the convolution epilogue's partial sums); the outputs of the skipped launch keep whatever their buffers held. */
int mrcnn_debug_bn_skip(int mask);
/* Measurement knobs of the channel-wise reductions (A/B in one process, tools/bn_plan_ab.py; the defaults are 1024, 4): most row
 * blocks = partial rows a reduction pass may use (also sizes mrcnn_bn_workspace_bytes: set it before the sizes are asked for), and
 * the channel quads one finalisation workgroup sums (4: 64 row slices x 16 channels; 1: 256 slices of one quad - slower). */
int mrcnn_debug_bn_plan(int red_cap, int fin_quads);
/* wino_v (nullable): caller-owned buffer of mrcnn_conv2d_winograd_v_bytes() bytes (0 = the layer does not take the
 * Winograd path).  The forward pass leaves its transformed input there and the filter-gradient pass of the same layer
 * reads it instead of transforming x again (same call geometry, same Winograd settings). */
size_t mrcnn_conv2d_winograd_v_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mrcnn_conv2d_fwd_f32(const float *x, const float *w, const float *bias, float *y, int N, int H,
                         int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu,
                         float *wino_v, void *ws, size_t ws_bytes, void *stream);
/* Forward with a rectangular kernel and per-axis padding: the (15,1) / (1,15) separable pairs of the Light-Head R-CNN
 * head (chainer_maskrcnn/model/head/light_roi_mask_head.py:29-44).  Workspace as mrcnn_conv2d_workspace_bytes() of the
 * same geometry with pad = max(pad_h, pad_w). */
/* Convolution feeding a training-mode BatchNorm (no bias, no ReLU: extractor/feature_pyramid_network.py:48-66, Chainer's
 * ResNet50Layers): the GEMM epilogue also leaves per-channel sums / sums of squares of every block of output rows in
 * bn_part (rows, 2, Cout); mrcnn_bn_train_fwd_stats_f32 finishes BatchNorm from them without a statistics pass over the
 * activation.  Winograd layers produce the same partials in their output transform (wino_v / ws as for
 * mrcnn_conv2d_fwd_f32).  mrcnn_conv2d_bnstats_rows = rows for this geometry, or 0 when the call would take a path without
 * the fused statistics (split-K or tail-split launches): use the plain entry points then. */
size_t mrcnn_conv2d_bnstats_rows(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mrcnn_conv2d_fwd_bnstats_f32(const float *x, const float *w, float *y, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                 int stride, int pad, float *bn_part, float *wino_v, void *ws, size_t ws_bytes, void *stream);
int mrcnn_conv2d_fwd_rect_f32(const float *x, const float *w, const float *bias, float *y, int N, int H, int W, int Cin,
                              int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int relu, void *ws,
                              size_t ws_bytes, void *stream);
/* relu_x (nullable, same shape as gx): the layer's input when it is the output of a ReLU; gx is then zeroed where
 * relu_x <= 0, i.e. the ReLU backward of the layer below is fused into this epilogue; with accumulate (ABI v7) the old value is
 * added first and the TOTAL is masked (the last contribution to a fan-out point applies the mask to all of them). */
/* wino_w (nullable, mrcnn_conv2d_winograd_w_bytes() bytes; only where that is > 0): the Winograd path reads gy ONCE
 * and leaves the filter-gradient GEMM's operand (A dy A^T) there for the mrcnn_conv2d_bwd_filter_f32 call of the same
 * layer; with wino_w, gbias (nullable, Cout) receives the bias gradient (column sums of gy; added to when
 * gbias_accumulate != 0) from the same read. */
size_t mrcnn_conv2d_winograd_w_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mrcnn_conv2d_bwd_data_f32(const float *gy, const float *w, float *gx, const float *relu_x, int N, int H, int W, int Cin,
                              int Cout, int KH, int KW, int stride, int pad, int accumulate, float *wino_w,
                              float *gbias, int gbias_accumulate, void *ws, size_t ws_bytes, void *stream);
size_t mrcnn_conv2d_bwd_filter_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                               int stride, int pad);
int mrcnn_conv2d_bwd_filter_f32(const float *x, const float *gy, float *gw, float *gbias, int N, int H,
                                int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int accumulate,
                                const float *wino_v, const float *wino_w,
                                void *ws, size_t ws_bytes, void *stream);
/* The two backward passes of a layer whose output gradient is zero on whole images of the batch (the rows of the mask branch that
 * the mask loss does not read).  active (nullable; n_active == N bytes on the device, else MRCNN_E_INVALID): active[n] == 0 is the
 * caller's promise that gy is all zero on image n.  The Winograd layers on the plane GEMMs then leave those images out of their
 * transforms and GEMMs (no launch changes its grid, plan or order of sums: a skipped term is an exact zero); every other path runs
 * the dense pass.  Results equal the plain entry points' up to the sign of zero; gx of an inactive image is zero, or unchanged with
 * accumulate.  A NULL active is the plain call.  mrcnn_active_rows_u8 writes the mask of a row-blocked batch on the device:
 * active[r] = (r % rows_per_block) < n_pos[r / rows_per_block] for r < n_blocks * rows_per_block. */
int mrcnn_conv2d_bwd_data_active_f32(const float *gy, const float *w, float *gx, const float *relu_x, int N, int H, int W, int Cin,
                                     int Cout, int KH, int KW, int stride, int pad, int accumulate, const unsigned char *active,
                                     int n_active, void *ws, size_t ws_bytes, void *stream);
int mrcnn_conv2d_bwd_filter_active_f32(const float *x, const float *gy, float *gw, float *gbias, int N, int H,
                                       int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int accumulate,
                                       const float *wino_v, const unsigned char *active, int n_active,
                                       void *ws, size_t ws_bytes, void *stream);
int mrcnn_active_rows_u8(const int32_t *n_pos, int n_blocks, int rows_per_block, unsigned char *active, void *stream);

/* ------------------------------------------------------------------------------------------
 * Backbone / head layer kernels (nn.hip), NHWC fp32, "(P, C)" = P pixels x C channels, C % 4 == 0.
 * Replace the cuDNN / CuPy kernels behind ResNet50Layers' BatchNormalization + ReLU + residual add,
 * F.max_pooling_2d(ksize=2) (cover_all), F.unpooling_2d(ksize=2, outsize) + add
 * (chainer_maskrcnn/model/extractor/feature_pyramid_network.py:48-66), the ReLUs and the
 * Deconvolution2D data movement of chainer_maskrcnn/model/head/fpn_roi_mask_head.py:65-83, and the
 * optimizer of train.py:107-109.
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_bn_workspace_bytes(int P, int C);
/* Training-mode BN: batch statistics over P, y = gamma*(x-mean)*invstd + beta (+ residual) (ReLU if
 * relu != 0); save_mean / save_invstd (C) are kept for backward; running_* (nullable) are updated with
 * Chainer's rule (decay, unbiased variance).
 * Channel counts: C % 4 == 0, and C / 4 either at most 256 or a multiple of 256 (C = 1024, 2048, ...): the reduction passes of
 * mrcnn_bn_train_fwd_f32, _bwd_f32, _stats_f32 / _fwd_pair_f32 without partial rows and _bwd_pair_f32 walk the channel groups 256 at a
 * time around workgroup barriers; every other count is MRCNN_E_INVALID before any launch (the forms fed by partial rows take it). */
int mrcnn_bn_train_fwd_f32(const float *x, const float *gamma, const float *beta, const float *residual,
                           float *y, float *save_mean, float *save_invstd, float *running_mean,
                           float *running_var, int P, int C, float eps, float decay, int relu, void *ws,
                           size_t ws_bytes, void *stream);
/* dz = relu ? gy*(y>0) : gy;  gx = BN backward of dz;  gres (nullable) = dz (gradient of the residual
 * input);  ggamma, gbeta (C) overwritten.  y may be NULL when relu != 0, the forward had no residual and beta is
 * given: the mask is then recomputed from x as gamma*(x-mean)*invstd + beta > 0 with the forward's exact expression
 * (bitwise the same mask, one HBM stream less).  beta is otherwise unused (nullable). */
int mrcnn_bn_train_fwd_stats_f32(const float *x, const float *part, int rows, const float *gamma, const float *beta,
                                 const float *residual, float *y, float *save_mean, float *save_invstd, float *running_mean,
                                 float *running_var, int P, int C, float eps, float decay, int relu, void *stream);
int mrcnn_bn_train_bwd_f32(const float *gy, const float *x, const float *y, const float *gamma, const float *beta,
                           const float *save_mean, const float *save_invstd, float *gx, float *gres,
                           float *ggamma, float *gbeta, int P, int C, int relu, void *ws, size_t ws_bytes,
                           void *stream);
/* (ABI v10) Two training-mode BatchNorms that meet in one residual sum - the main branch and the projection shortcut of a ResNet bottleneck
 * (extractor/feature_pyramid_network.py:48-66; Chainer's BottleneckA): y = relu(BN_a(xa) + BN_b(xb)).  Statistics of each layer as in the
 * single-layer entry points (part_x / rows_x: the partial rows its convolution left behind, mrcnn_conv2d_fwd_bnstats_f32; NULL / 0 = a
 * statistics pass over the tensor through ws of mrcnn_bn_workspace_bytes()), then ONE apply kernel: the shortcut's BatchNorm output is never
 * written.  The backward pair: dz = y ? gy * (y > 0) : gy (y NULL = gy arrives masked); gxa / gxb = BatchNorm backward of dz through each
 * layer (ws of mrcnn_bn_pair_workspace_bytes()); the masked gradient is never written either.  Same bits as the layer-by-layer sequence
 * mrcnn_bn_train_fwd(_stats)_f32(xb -> r), mrcnn_bn_train_fwd(_stats)_f32(xa, residual r, relu) and its two mrcnn_bn_train_bwd_f32 calls:
 * 5 passes over a (P, C) tensor fewer per projection block and step. */
/* (ABI v10) conv -> BatchNorm -> ReLU -> conv 3x3 without the normalised activation (the middle of a ResNet bottleneck,
 * extractor/feature_pyramid_network.py:48-66): mrcnn_bn_train_stats_f32 finishes the statistics of the first convolution's output (partial rows
 * from its epilogue, or NULL / 0 = a statistics pass through ws) and updates the running statistics - no apply kernel; the consumer's Winograd
 * input transform applies gamma * ((x - mean) * invstd) + beta and the ReLU to every tap as it loads it (taps outside the image stay zero):
 * mrcnn_conv2d_fwd_inbn_f32 (bn_part nullable: also the statistics partials of ITS output, as mrcnn_conv2d_fwd_bnstats_f32) and
 * mrcnn_conv2d_bwd_filter_inbn_f32 (wino_v as mrcnn_conv2d_bwd_filter_f32).  Same bits as the materialised sequence; 2 passes over the
 * (P, C) activation and one launch fewer.  Only where mrcnn_conv2d_inbn_ok() != 0 (3x3 / stride 1 / pad 1 geometries whose forward and
 * filter-gradient passes both take the Winograd path under the process settings in force); the entry points refuse other geometries. */
int mrcnn_bn_train_stats_f32(const float *x, const float *part, int rows, float *save_mean, float *save_invstd, float *running_mean,
                             float *running_var, int P, int C, float eps, float decay, void *ws, size_t ws_bytes, void *stream);
int mrcnn_conv2d_inbn_ok(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mrcnn_conv2d_fwd_inbn_f32(const float *x, const float *in_gamma, const float *in_beta, const float *in_mean, const float *in_invstd,
                              const float *w, float *y, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                              float *bn_part, float *wino_v, void *ws, size_t ws_bytes, void *stream);
int mrcnn_conv2d_bwd_filter_inbn_f32(const float *x, const float *in_gamma, const float *in_beta, const float *in_mean,
                                     const float *in_invstd, const float *gy, float *gw, int N, int H, int W, int Cin, int Cout, int KH,
                                     int KW, int stride, int pad, int accumulate, const float *wino_v, void *ws, size_t ws_bytes,
                                     void *stream);
size_t mrcnn_bn_pair_workspace_bytes(int P, int C);
int mrcnn_bn_train_fwd_pair_f32(const float *xa, const float *part_a, int rows_a, const float *gamma_a, const float *beta_a,
                                float *mean_a, float *invstd_a, float *run_mean_a, float *run_var_a, const float *xb,
                                const float *part_b, int rows_b, const float *gamma_b, const float *beta_b, float *mean_b,
                                float *invstd_b, float *run_mean_b, float *run_var_b, float *y, int P, int C, float eps, float decay,
                                void *ws, size_t ws_bytes, void *stream);
int mrcnn_bn_train_bwd_pair_f32(const float *gy, const float *y, const float *xa, const float *xb, const float *gamma_a,
                                const float *mean_a, const float *invstd_a, const float *gamma_b, const float *mean_b,
                                const float *invstd_b, float *gxa, float *gxb, float *ggamma_a, float *gbeta_a, float *ggamma_b,
                                float *gbeta_b, int P, int C, void *ws, size_t ws_bytes, void *stream);
/* Inference-mode BN with the running statistics (chainer.config.train == False, maskrcnn.py:171-172). */
int mrcnn_bn_infer_fwd_f32(const float *x, const float *gamma, const float *beta, const float *mean,
                           const float *var, const float *residual, float *y, int P, int C, float eps, int relu,
                           void *stream);
int mrcnn_relu_bwd_f32(const float *gy, const float *y, float *gx, size_t n, void *stream);
int mrcnn_add_f32(const float *a, const float *b, float *out, size_t n, void *stream);
int mrcnn_maxpool2x2_fwd_f32(const float *x, float *y, int N, int H, int W, int C, void *stream);
int mrcnn_maxpool2x2_bwd_f32(const float *x, const float *gy, float *gx, int N, int H, int W, int C, void *stream);
/* Legacy variants (forward only): F.max_pooling_2d(ksize=3, stride=2) with cover_all
 * (chainer_maskrcnn/model/extractor/c4_backbone.py:20; Ho = (H-3+1)/2 + 1), global average pooling of x (R,P,C) -> (R,C)
 * (model/head/resnet_roi_mask_head.py:65) and a stand-alone ReLU (x == y allowed). */
int mrcnn_maxpool3x3s2_fwd_f32(const float *x, float *y, int N, int H, int W, int C, void *stream);
int mrcnn_global_avg_pool_fwd_f32(const float *x, float *y, int R, int P, int C, void *stream);
int mrcnn_relu_fwd_f32(const float *x, float *y, size_t n, void *stream);
/* out (N,H,W,C) = nearest-2x(top (N,Ht,Wt,C)) cropped + lat;  backward: gtop (+)= 2x2 block sums of gout. */
int mrcnn_upsample2x_add_fwd_f32(const float *top, const float *lat, float *out, int N, int H, int W, int Ht,
                                 int Wt, int C, void *stream);
int mrcnn_upsample2x_bwd_f32(const float *gout, float *gtop, int N, int H, int W, int Ht, int Wt, int C,
                             int accumulate, void *stream);
/* Backward of the lattice subsampling x[:, ::s, ::s] (strided 1x1 convolutions): gx (N,H,W,C).  relu_x (nullable, ABI v7; shape of
 * gx): the lattice positions are zeroed where relu_x <= 0 after the accumulation - the ReLU backward of the layer that produced the
 * subsampled tensor, applied where its gradient is written last (positions off the lattice keep gx's contents). */
int mrcnn_subsample_bwd_f32(const float *gsub, float *gx, int N, int H, int W, int C, int stride, int accumulate,
                            const float *relu_x, void *stream);
/* 2x2/2 deconvolution data movement: (N,H,W,[2][2][C]) <-> (N,2H,2W,C); inverse != 0 is the backward. */
int mrcnn_pixel_shuffle2x_f32(const float *src, const float *bias, float *dst, int N, int H, int W, int C, int inverse,
                              void *stream);      /* bias (C, nullable) is added in the forward direction */
/* Algebraic merge of the mask / keypoint branch's last two layers: the reference has no non-linearity between the
 * 2x2/2 deconvolution and the final 1x1 convolution (head/fpn_roi_mask_head.py:83, fpn_roi_keypoint_head.py:93), so
 * conv2(deconv1(x)) is one 2x2/2 deconvolution to K2 channels (4x fewer MACs at 28x28, no (R,28,28,C) intermediate).
 *   wd (4*C, Cin) rows (a*2+b)*C + o;  bd (C);  w2 (K2, ld2 >= C) (columns >= C are channel padding and are left
 *   untouched in gw2);  b2 (K2, nullable)
 *   fwd: wm (4*K2, Cin) rows (a*2+b)*K2 + k = W2 * Wd[ab];  bm (K2) = b2 + W2 * bd
 *   bwd: G (4*K2, Cin), gb4 (4*K2) = filter / bias gradient of the merged layer  ->  gwd, gbd, gw2, gb2 (nullable),
 *        all overwritten; exact gradients of the un-merged parameters, fixed summation order. */
int mrcnn_deconv_merge_fwd_f32(const float *wd, const float *bd, const float *w2, const float *b2, float *wm,
                               float *bm, int C, int Cin, int K2, int ld2, void *stream);
int mrcnn_deconv_merge_bwd_f32(const float *G, const float *gb4, const float *wd, const float *bd,
                               const float *w2, float *gwd, float *gbd, float *gw2, float *gb2, int C,
                               int Cin, int K2, int ld2, void *stream);
/* Bilinear x2 with corner alignment (Chainer F.resize_images, chainer_maskrcnn/model/head/fpn_roi_keypoint_head.py:
 * 80-81,109): x (N,H,W,C) -> y (N,2H,2W,C); bwd is the exact adjoint (owner-computes, no atomics). */
int mrcnn_bilinear2x_fwd_f32(const float *x, float *y, int N, int H, int W, int C, void *stream);
int mrcnn_bilinear2x_bwd_f32(const float *gy, float *gx, int N, int H, int W, int C, void *stream);
/* x (N,3,H,W) NCHW -> y (N,H,W,4) NHWC with a zero 4th channel (the image layer's operand layout). */
int mrcnn_image_nchw3_to_nhwc4_f32(const float *x, float *y, int N, int H, int W, void *stream);
/* Device side of the training Transform (train.py:21-37; chainer_maskrcnn/dataset/transforms.py is the host form):
 * the raw uint8 image (H,W,3) / instance masks (G,H,W) are resized into planes of a zero-initialised padded batch tensor
 * (dst_h x dst_w per plane; rows < oh and columns < ow are written).  cv2.resize INTER_LINEAR / INTER_NEAREST
 * coordinate rules; the image is divided by `div` (255 = MaskRCNN.prepare, maskrcnn.py:274). */
int mrcnn_image_resize_u8_f32(const uint8_t *src, int H, int W, float *dst, int oh, int ow, int dst_h, int dst_w,
                              float div, void *stream);
int mrcnn_mask_resize_nearest_u8(const uint8_t *src, int G, int H, int W, uint8_t *dst, int oh, int ow, int dst_h,
                                 int dst_w, void *stream);
/* MaskRCNN.prepare (chainer_maskrcnn/model/maskrcnn.py:261-276): the float32 CHW image (C,H,W) resized with cv2's
 * INTER_LINEAR float rule (what chainercv.transforms.resize calls) into planes of dst_h x dst_w, then divided by div. */
int mrcnn_image_resize_f32(const float *src, int C, int H, int W, float *dst, int oh, int ow, int dst_h, int dst_w,
                           float div, void *stream);
/* n uint32 sampler keys from a counter-based hash of (seed, index). */
int mrcnn_random_keys_u32(uint32_t *out, size_t n, unsigned long long seed, void *stream);
/* Same with the seed in device memory (state[0]); the call also advances the state, so a replayed HIP graph draws
 * fresh keys every time. */
int mrcnn_random_keys_dev_u32(uint32_t *out, size_t n, unsigned long long *state, void *stream);
/* g += wd*p; v = momentum*v - lr*g; p += v  over a flat parameter buffer (train.py:107-109). */
int mrcnn_sgd_momentum_wd_f32(float *p, const float *g, float *v, size_t n, float lr, float momentum,
                              float weight_decay, void *stream);

/* ------------------------------------------------------------------------------------------
 * (ABI v9) One whole ResNet bottleneck per call.  Replaces the Python-issued chain of Chainer's ResNet50Layers building block
 * (BottleneckA / BottleneckB: conv1x1 -> BN -> ReLU -> conv3x3 -> BN -> ReLU -> conv1x1 -> BN (+ shortcut, itself conv1x1 -> BN in
 * the first block of a stage) -> ReLU) as the reference runs it in training mode, extractor/feature_pyramid_network.py:22,48-66, and its
 * backward - the host side of the updater loop, train.py:117-132.  The call ENQUEUES exactly the launches the separate entry points
 * above would (mrcnn_conv2d_fwd_bnstats_f32 / mrcnn_conv2d_fwd_f32, mrcnn_bn_train_fwd_stats_f32 / mrcnn_bn_train_fwd_f32,
 * mrcnn_bn_train_bwd_f32, mrcnn_conv2d_bwd_filter_f32, mrcnn_conv2d_bwd_data_f32, mrcnn_subsample_bwd_f32, mrcnn_add_f32), in the same
 * order with the same operands: the results are the same bits; what changes is the host cost (one foreign call and two or three
 * allocations per block instead of ~25 calls and ~20 allocations).
 *
 * Descriptor (host memory, read during the call only).  Channel counts are the padded ones of the tensors (multiples of 32).
 *   x (N,H,W,cin) NHWC;  conv1: 1x1 stride `stride` cin->mid;  conv2: 3x3 pad 1 mid->mid;  conv3: 1x1 mid->cout;
 *   project != 0: shortcut conv4 1x1 stride `stride` cin->cout + bn4, else identity (cin == cout, stride 1).
 *   w[i] filters (Cout,KH,KW,Cin); gamma/beta/run_mean/run_var of bn1..bn4; gw/ggamma/gbeta: where the backward writes the gradients.
 *   fwd_split: -1 = the process setting (mrcnn_conv2d_set_split_operands); 0..3 = that arithmetic for the FORWARD convolutions of this
 *   call (the setting is restored before return).
 * Forward: mrcnn_bottleneck_fwd_plan fills `plan` (offsets of the saved tensors inside the caller's arena: pre-BN / post-BN
 * activations, kept Winograd input transforms, statistics partials, saved mean / invstd) and returns the arena and scratch sizes for
 * the CURRENT convolution settings; mrcnn_bottleneck_fwd_f32 follows that plan.  The arena is what the backward needs: keep it, with the
 * plan, until mrcnn_bottleneck_bwd_f32 has been enqueued.  y (N,Ho,Wo,cout) is the block's output.
 * Backward: gy = gradient of y.  gy_masked != 0: gy already carries the block's output ReLU mask (its producer applied it), the shortcut
 * gradient is gy itself; else g_r (N,Ho,Wo,cout, required) receives the masked gradient.  The block's input gradient:
 *   identity shortcut: accumulated into gx_acc when given (gx_acc = g_r + gx_acc first), else into g_r / gy IN PLACE (as the Python chain);
 *   projection: accumulated into gx_acc when given, else written to gx_new (N,H,W,cin, required then).
 * mask_gx != 0: that gradient is zeroed where x <= 0 (x is a ReLU output: the ReLU backward of the block before).
 * side_stream (nullable): the four filter gradients are enqueued there, each behind an event recorded on `stream` when its operands are
 * complete (the library keeps a small pool of timing-disabled events per device for this; no device memory); NULL = everything on
 * `stream`.  ws_side is the side stream's own scratch.  The caller joins the side stream when it needs the filter gradients.
 * ---------------------------------------------------------------------------------------- */
typedef struct mrcnn_bottleneck {
    int32_t N, H, W;
    int32_t cin, mid, cout;
    int32_t stride, project;
    int32_t fwd_split;
    float eps, decay;
    const float *w[4];
    const float *gamma[4];
    const float *beta[4];
    float *run_mean[4];
    float *run_var[4];
    float *gw[4];
    float *ggamma[4];
    float *gbeta[4];
} mrcnn_bottleneck_t;

enum { MRCNN_BN_H1 = 0, MRCNN_BN_A1, MRCNN_BN_H2, MRCNN_BN_A2, MRCNN_BN_H3, MRCNN_BN_H4, MRCNN_BN_R,
       MRCNN_BN_V = 7 /* +0..3 */, MRCNN_BN_PART = 11 /* +0..3 */, MRCNN_BN_MEAN = 15 /* +0..3 */, MRCNN_BN_INVSTD = 19 /* +0..3 */,
       MRCNN_BN_SLOTS = 23 };

typedef struct mrcnn_bottleneck_plan {
    uint64_t arena_bytes;               /* forward arena */
    uint64_t ws_bytes;                  /* forward scratch on `stream` */
    uint64_t off[MRCNN_BN_SLOTS];       /* byte offsets into the arena (256-B aligned); unused slots 0 */
    uint64_t v_bytes[4];                /* kept Winograd input transform of conv1..4 (0: none) */
    int32_t part_rows[4];               /* statistics partial rows of conv1..4 (0: BatchNorm runs its own statistics pass) */
} mrcnn_bottleneck_plan_t;

/* measurement: 0 = the composite calls materialise bn1's output as before (A/B of mrcnn_conv2d_fwd_inbn_f32); default 1 */
int mrcnn_debug_bottleneck_inbn(int on);
int mrcnn_bottleneck_fwd_plan(const mrcnn_bottleneck_t *b, mrcnn_bottleneck_plan_t *plan);
int mrcnn_bottleneck_fwd_f32(const mrcnn_bottleneck_t *b, const mrcnn_bottleneck_plan_t *plan, const float *x, float *y,
                             void *arena, size_t arena_bytes, void *ws, size_t ws_bytes, void *stream);
/* sizes3 (host, 3 x size_t): backward arena (the intermediate gradients), scratch on `stream`, scratch on `side_stream` */
int mrcnn_bottleneck_bwd_sizes(const mrcnn_bottleneck_t *b, size_t *sizes3);
int mrcnn_bottleneck_bwd_f32(const mrcnn_bottleneck_t *b, const mrcnn_bottleneck_plan_t *plan, const float *x, const float *y,
                             const void *fwd_arena, const float *gy, int gy_masked, float *g_r, float *gx_acc, float *gx_new,
                             int mask_gx, void *arena, size_t arena_bytes, void *ws_main, size_t ws_main_bytes, void *ws_side,
                             size_t ws_side_bytes, void *stream, void *side_stream);

/* ------------------------------------------------------------------------------------------
 * Losses (loss.hip).  Replace F.softmax_cross_entropy, _fast_rcnn_loc_loss/_smooth_l1_loss and
 * calc_mask_loss (chainer_maskrcnn/model/fpn_maskrcnn_train_chain.py:83-85,100-106; train.py:50-58;
 * train_keypoints.py:21-27).  loss_out is 2 floats on the device: [0] = loss, [1] = normaliser.
 * gx (nullable) receives d loss / d logits.
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_loss_workspace_bytes(void);
/* softmax_ce: element (r, j) of the logical (M, K) logits lives at (r / A) * gs + (r % A) * rs + j * es floats (gx: ggs, grs, ges).
 * Rows that are CHANNELS of an NHWC (G, K, C) tensor (rs = 1, es = C, gs = K * C, A <= C, C a multiple of 4 that divides 1024, K >= 64:
 * the keypoint loss of train_keypoints.py:21-27, 17 heat maps in 32 padded channels) take a coalesced kernel - one workgroup per group,
 * float4 loads over the (position, channel) plane, loss and gradient from one launch - which writes EVERY element of gx (zeros in the
 * channels >= A and in the ignored rows); on the other paths gx receives the K (Kfill) columns of its M rows only. */
/* 1 when mrcnn_softmax_ce_f32 called with these maps writes EVERY element of gx itself (its channel-interleaved path: the keypoint loss),
 * so that the caller need not zero-fill gx; 0 = the strided path writes only the K columns of the M rows.  The library's own dispatch
 * predicate, exported (one source of truth). */
int mrcnn_softmax_ce_fills_gx(int M, int K, int A, long long gs, long long rs, long long es, long long ggs, long long grs, long long ges,
                              int Kfill);
int mrcnn_softmax_ce_f32(const float *x, int A, long long gs, long long rs, long long es, const int32_t *t,
                         int M, int K, int ignore_label, float *loss_out, float *gx, long long ggs,
                         long long grs, long long ges, int Kfill, void *ws, size_t ws_bytes, void *stream);
int mrcnn_smooth_l1_f32(const float *x, int ldx, const float *t, const int32_t *label, int M, float sigma,
                        float *loss_out, float *gx, int ldg, int gfill, void *ws, size_t ws_bytes, void *stream);
int mrcnn_mask_bce_f32(const float *x, const int32_t *gt, const int32_t *label, int Rm, int HW, int Cm,
                       float *loss_out, float *gx, void *ws, size_t ws_bytes, void *stream);
/* Building blocks of a USER-SUPPLIED mask_loss_fun (the reference passes a plain Python function: train.py:50-58,98;
 * train_keypoints.py:21-27): the host layer wraps them as autograd functions (chainer_maskrcnn/functions/loss.py) so
 * the bodies of those functions run on device tensors.
 *   sigmoid_ce      chainer.functions.sigmoid_cross_entropy(x, t): normalize=True, ignore label -1, mean; n elements
 *   select_channel  roi_cls_mask[xp.arange(R), idx] on an NCHW tensor (R,C,HW): y (R,HW); negative idx wraps like NumPy;
 *                   backward != 0: src = gy (R,HW), dst = gx (R,C,HW) fully written (zeros elsewhere)
 *   nhwc_nchw       (R,HW,Cp) NHWC with Cp >= C padded channels -> (R,C,HW) NCHW; inverse != 0: back, padding zeroed
 *   scale_by_dev    x *= scale[0] with the scalar in device memory (upstream gradient of a loss output) */
int mrcnn_sigmoid_ce_f32(const float *x, const int32_t *t, long long n, float *loss_out, float *gx, void *ws,
                         size_t ws_bytes, void *stream);
int mrcnn_select_channel_f32(const float *src, const int32_t *idx, int R, int C, int HW, float *dst, int backward,
                             void *stream);
int mrcnn_nhwc_nchw_f32(const float *src, float *dst, int R, int HW, int Cp, int C, int inverse, void *stream);
int mrcnn_scale_by_dev_f32(float *x, size_t n, const float *scale, void *stream);
/* out[0] = sum of n (loss, normaliser) pairs' losses: the un-weighted total of fpn_maskrcnn_train_chain.py:106 */
int mrcnn_loss_total_f32(const float *losses, int n, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * IoU-based box regression losses on the DECODED box (box_loss.hip; no counterpart in the reference, which has the smooth L1 on the
 * encoded deltas only).  A drop-in for mrcnn_smooth_l1_f32: same predictions, targets, labels, normaliser and gradient-buffer contract.
 *   x (M, ldx >= 4): the predicted deltas of row r at x[r * ldx .. + 4) (the caller offsets the pointer to its first loc column)
 *   t (M,4): the encoded, normalised targets of the target creators
 *   rois (roi_period,4) (y1,x1,y2,x2): row r is relative to rois[r % roi_period] (the head: roi_period = M, the sampled RoIs; the RPN:
 *     roi_period = A, the anchors every image of the batch shares)
 *   label (M) int32: rows with label > 0 carry loss; the normaliser is #(label >= 0), at least 1
 *   mean4, std4: HOST arrays of 4 floats, read during the call: d = v * std + mean for predictions and targets alike
 * Both boxes are decoded with the arithmetic of mrcnn_detect_decode_f32 without un-scaling and clipping: centre = d_yx * size + centre,
 * size = expf(d_hw) * size, corners = centre -+ size / 2.  The PREDICTED d_h, d_w are clamped above at log(1000 / 16) before expf: a
 * clamped coordinate has gradient exactly 0, a coordinate at the bound itself passes it; the target is not clamped.  With eps = 1e-7, P the
 * prediction, G the target, ih = max(0, min(P.y2, G.y2) - max(P.y1, G.y1)) (iw likewise), inter = ih * iw, union = aP + aG - inter + eps,
 * iou = inter / union, ch and cw the sides of the enclosing box:
 *   MRCNN_BOX_LOSS_GIOU  L = 1 - iou + (ch * cw - union) / (ch * cw + eps)
 *   MRCNN_BOX_LOSS_DIOU  L = 1 - iou + rho2 / (ch^2 + cw^2 + eps), rho2 = the squared distance of the two centres
 *   MRCNN_BOX_LOSS_CIOU  DIoU + alpha * v, v = 4 / pi^2 * (atan(wG / (hG + eps)) - atan(wP / (hP + eps)))^2, alpha = v / (1 - iou + v + eps)
 *                        taken as a constant in the gradient
 * loss_out[0] = weight * (sum of L over the rows with label > 0) / count, loss_out[1] = count.  gx (nullable; row stride ldg):
 * gx[r * ldg .. + 4) = d loss / d x for d loss = 1 (weight and 1 / count included), zeros in rows with label <= 0; columns 4 .. gfill - 1
 * of every row are zero-filled and nothing outside [0, max(4, gfill)) of a row is written.  A tie of a min / max splits the derivative
 * evenly; the overlap's clamp at 0 passes it where the overlap is positive.  ws: mrcnn_loss_workspace_bytes() bytes.
 * Three launches (block partials, fixed-order finalize, gradient; two without gx), no float atomics: bit-identical from run to run.  No
 * host synchronisation, no allocation.  M == 0 writes loss 0, count 1.  Errors, before any launch: MRCNN_E_INVALID for M > 0 with a NULL
 * x / t / rois / label, M < 0, ldx < 4, roi_period <= 0, a kind outside 1..3, a NULL loss_out / ws / mean4 / std4, ldg below
 * max(4, gfill) with gx given; MRCNN_E_WORKSPACE for a short workspace.
 * ---------------------------------------------------------------------------------------- */
enum { MRCNN_BOX_LOSS_GIOU = 1, MRCNN_BOX_LOSS_DIOU = 2, MRCNN_BOX_LOSS_CIOU = 3 };
int mrcnn_box_iou_loss_f32(const float *x, int ldx, const float *t, const float *rois, int roi_period, const int32_t *label, int M,
                           int kind, const float *mean4, const float *std4 /* host */, float weight, float *loss_out, float *gx, int ldg,
                           int gfill, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * RPN proposal path (rpn.hip).  Replaces the transposes/concats and the ChainerCV ProposalCreator +
 * non_maximum_suppression + map_rois_to_fpn_levels calls of
 * chainer_maskrcnn/model/rpn/multilevel_region_proposal_network.py:16-31,133-164.
 *   head (N,HW,Cp): channels [0,4A) loc, [4A,6A) score;  locs (N,Atot,4);  scores (N,Atot,2)
 *   rois (N*n_post,4) yx, zero padded;  roi_indices (N*n_post) = image or -1;  levels f32;  n_rois (N)
 *   dbg_* (nullable): anchor index of each pre-NMS box in sort order (N*n_pre), NMS keep list
 *   (N*n_post, indices into the sort order), pre-NMS count (N).
 *   per_image (nullable, device, (N,3) f32 = h, w, min_size * scale): a padded batch of images of different sizes - every
 *   image's boxes are clipped to its own size and filtered with its own scaled min_size, as the reference (batch 1 per
 *   process, rpn/...:156-164: img_size and scale of THAT image) does; null = img_h / img_w / min_size for all.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_rpn_pack_f32(const float *head, int N, int HW, int Cp, int A, float *locs, float *scores, int a_off,
                       int Atot, void *stream);
int mrcnn_rpn_unpack_grad_f32(const float *glocs, const float *gscores, int N, int HW, int Cp, int A,
                              float *ghead, int a_off, int Atot, void *stream);
/* (ABI v10) The same for ALL pyramid levels in one launch each way (heads / gheads: L host-side device pointers, HWs: positions per level;
 * level l's anchors follow level l-1's in the concatenated axis, sum(HWs) * A == Atot): the concat of rpn/...:143-152 and its backward. */
int mrcnn_rpn_pack_levels_f32(const float *const *heads, const int *HWs, int L, int N, int Cp, int A, float *locs, float *scores,
                              int Atot, void *stream);
int mrcnn_rpn_unpack_grad_levels_f32(const float *glocs, const float *gscores, float *const *gheads, const int *HWs, int L, int N,
                                     int Cp, int A, int Atot, void *stream);
size_t mrcnn_rpn_proposals_workspace_bytes(int N, int A, int n_pre, int n_post);
int mrcnn_rpn_proposals_f32(const float *locs, const float *scores, const float *anchors, int N, int A,
                            float img_h, float img_w, float min_size, const float *per_image, int n_pre, int n_post, float nms_thresh,
                            float *rois, int32_t *roi_indices, float *levels, int32_t *n_rois,
                            int32_t *dbg_sorted_anchor, int32_t *dbg_keep, int32_t *dbg_n_pre, void *ws,
                            size_t ws_bytes, void *stream);
size_t mrcnn_nms_workspace_bytes(int n);
int mrcnn_nms_f32(const float *boxes, int n, float thresh, int max_keep, int32_t *keep, int32_t *n_keep,
                  void *ws, size_t ws_bytes, void *stream);
int mrcnn_map_rois_to_fpn_levels_f32(const float *rois, int R, int k_min, int k_max, float *levels, void *stream);
/* out (M,2) = softmax over the 2 class scores of in (M,2): ChainerCV's single-level RegionProposalNetwork (the 'c4'
 * backbone, chainer_maskrcnn/model/maskrcnn.py:60-69) ranks its proposals by the foreground PROBABILITY. */
int mrcnn_softmax2_f32(const float *in, float *out, size_t M, void *stream);

/* ------------------------------------------------------------------------------------------
 * Target creators (targets.hip).  Replace chainer_maskrcnn/utils/proposal_target_creator.py:26-137
 * (host NumPy + cv2) and ChainerCV's AnchorTargetCreator (model/fpn_maskrcnn_train_chain.py:81-82).
 * Per image i the sampler owns rows [i*n_sample, (i+1)*n_sample): positives first, then negatives,
 * then padding (label -1).  keys: uint32 random numbers, (N, roi_cap + gt_cap) / (N, A).
 * proposal_target, reference-order mode: pos_order / neg_order (both or neither; (N, n_sample) int32) replace the keys -
 * row j of the positives is the candidate of RANK pos_order[j] among the foreground candidates in ascending index order,
 * which is np.random.choice(pos_index, size, replace=False) = pos_index[permutation(len)[:size]]
 * (utils/proposal_target_creator.py:63-78) when the host draws the permutation; n_cand (nullable, (N,2)) returns the
 * candidate-set sizes the host needs for that draw.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_proposal_target_f32(const float *rois, const float *roi_levels, const int32_t *n_rois, int roi_cap,
                              const float *gt_boxes, const int32_t *gt_labels, const int32_t *n_gt, int gt_cap,
                              const uint32_t *keys, int N, int n_sample, int n_pos_max, float pos_iou_thresh,
                              float neg_iou_thresh_hi, float neg_iou_thresh_lo, const float *loc_mean4,
                              const float *loc_std4, float *sample_roi, float *rois_xy5, int32_t *sample_levels,
                              float *gt_roi_loc, int32_t *gt_roi_label, int32_t *gt_assign, int32_t *sample_src,
                              int32_t *n_pos, int32_t *n_sampled, const int32_t *pos_order, const int32_t *neg_order,
                              int32_t *n_cand, void *stream);
int mrcnn_mask_target_u8(const unsigned char *masks, int N, int gt_cap, int H, int W, const float *sample_roi,
                         const int32_t *gt_assign, const int32_t *n_pos, int n_sample, int pos_cap, int mask_size,
                         int32_t *gt_roi_mask, void *stream);
/* inplace_quirk != 0 reproduces the reference's in-place mutation of the gt keypoints (a gt assigned to several
 * positives is transformed again from its already-transformed coordinates, in sample order). */
int mrcnn_keypoint_target_f32(const float *keypoints, int N, int gt_cap, int K, const float *sample_roi,
                              const int32_t *gt_assign, const int32_t *n_pos, int n_sample, int pos_cap,
                              int mask_size, int inplace_quirk, int32_t *gt_roi_kp, void *stream);
/* n_gt[i] = number of labels[i, :] >= 0: the per-image gt counts of a padded batch (Chainer concat_examples pads with
 * -1; dataset/loader.py does the same), valid rows first.  Used when the caller passes no counts (train.py:117-125). */
int mrcnn_count_valid_labels_i32(const int32_t *labels, int N, int G, int32_t *n_gt, void *stream);
/* per_image_hw (nullable, device, (N,2) f32): each image's own (h, w) for the "anchor inside the image" test of a padded
 * batch; null = img_h / img_w for all images. */
size_t mrcnn_anchor_target_workspace_bytes(int N, int A);
int mrcnn_anchor_target_f32(const float *anchors, int A, const float *gt_boxes, const int32_t *n_gt, int gt_cap,
                            int N, float img_h, float img_w, const float *per_image_hw, const uint32_t *keys, int n_sample,
                            float pos_iou_thresh, float neg_iou_thresh, float pos_ratio, int do_sample,
                            float *gt_rpn_loc, int32_t *gt_rpn_label, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Inference post-processing (predict.hip).  Replace the host code of
 * chainer_maskrcnn/model/maskrcnn.py:178-210 (decode + softmax), :278-312 (_suppress: per-class score filter +
 * ChainerCV NMS) and :231-246 (sigmoid, channel pick, cv2.resize to the box, threshold, paste).
 *   rois (R,4) yx in network-input pixels; box_out (R,ld): columns [0,n_class) scores, [loc0,loc0+4) class-agnostic loc
 *   cls_bbox (R,4) yx in original-image pixels; prob (R,n_class)
 *   keep_idx (n_class,R) int32: RoI indices kept for class l in selection (descending score) order; keep_cnt (n_class)
 *   mask_logits (D,S,S,Cm) NHWC; label (D) 0-based class = mask channel; bbox (D,4); out (D,H,W) uint8 {0,1}
 * ---------------------------------------------------------------------------------------- */
int mrcnn_detect_decode_f32(const float *rois, int R, const float *box_out, int ld, int n_class, int loc0,
                            float scale, const float *loc_mean4, const float *loc_std4, float size_h, float size_w,
                            float *cls_bbox, float *prob, void *stream);
int mrcnn_class_nms_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end,
                        float score_thresh, float nms_thresh, int32_t *keep_idx, int32_t *keep_cnt, void *stream);
int mrcnn_mask_paste_f32(const float *mask_logits, int D, int S, int Cm, const int32_t *label, const float *bbox,
                         int H, int W, unsigned char *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mask-IoU counts of the instance-segmentation evaluator (evaluate.hip).  Replace the host NumPy of ChainerCV's mask_iou
 * (chainercv/evaluations/eval_instance_segmentation_voc.py via chainercv/utils/mask/mask_iou.py; reference evaluator.py).
 *   a (Da,HW), b (Db,HW) uint8, contiguous rows (no alignment needed); any nonzero byte is a set pixel (torch.bool, mask_paste)
 *   a_label (Da), b_label (Db) int32: both NULL or both given; given = pairs with different labels get inter 0, no word work
 *   inter (Da,Db), area_a (Da), area_b (Db) int32: exact pixel counts (|a_i & b_j|, |a_i|, |b_j|), independent of the launch split
 *   ws: device scratch of mrcnn_mask_iou_workspace_bytes(Da, Db, HW) bytes (the bit-packed masks)
 * Da == 0 or Db == 0 is valid (the areas of the other side are written).  Errors, before any launch: MRCNN_E_INVALID for a
 * negative size, a NULL pointer of a non-empty side, or one label array only; MRCNN_E_WORKSPACE for a short workspace.
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_mask_iou_workspace_bytes(int Da, int Db, int HW);
int mrcnn_mask_iou_counts_u8(const unsigned char *a, int Da, const int32_t *a_label, const unsigned char *b, int Db,
                             const int32_t *b_label, int HW, void *ws, size_t ws_bytes, int32_t *inter, int32_t *area_a,
                             int32_t *area_b, void *stream);

/* ------------------------------------------------------------------------------------------
 * Boundary-IoU counts of the COCO evaluator's Boundary AP (evaluate.hip; Cheng et al., "Boundary IoU", CVPR 2021).  The boundary
 * band of a mask M is B = M & ~E, E = M eroded `dilation` times by a 3 x 3 block of ones with everything outside the image
 * background: E[y, x] = 1 iff M is 1 on the whole (2 d + 1) x (2 d + 1) square around (y, x) and that square lies inside the image.
 *   a (Da,H,W), b (Db,H,W) uint8, contiguous (no alignment needed); any nonzero byte is a set pixel
 *   a_label, b_label: as in mrcnn_mask_iou_counts_u8; cross-label pairs get 0 in inter and binter and do no word work
 *   dilation: the band width d, 1 <= d <= 63 (the host's rule: evaluations.boundary_dilation)
 *   inter, area_a, area_b: the mask counts, equal to those of mrcnn_mask_iou_counts_u8 on the same inputs
 *   binter (Da,Db), barea_a (Da), barea_b (Db) int32: |B(a_i) & B(b_j)|, |B(a_i)|, |B(b_j)|, exact, independent of the launch split
 *   ws: device scratch of mrcnn_mask_boundary_workspace_bytes(Da, Db, H, W) bytes (the row-aligned packed masks and bands)
 * mrcnn_mask_boundary_words_u8 is the first stage alone: bwords (D,H,ceil(W/64)) 64-bit words, bit k of word w of a row = band
 * pixel 64 w + k, tail bits zero; ws of mrcnn_mask_boundary_workspace_bytes(D, 0, H, W) bytes.
 * Empty sides (Da == 0, Db == 0, H * W == 0) are valid (the outputs of the other side are written, the rest zeroed).  Errors, before
 * any launch: MRCNN_E_INVALID for a negative size, dilation < 1, a NULL pointer of a non-empty side, or one label array only;
 * MRCNN_E_UNSUPPORTED for dilation > 63 or H * W > 2^31 - 1; MRCNN_E_WORKSPACE for a short workspace.
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_mask_boundary_workspace_bytes(int Da, int Db, int H, int W);
int mrcnn_mask_boundary_words_u8(const unsigned char *masks, int D, int H, int W, int dilation, void *ws, size_t ws_bytes,
                                 void *bwords, void *stream);
int mrcnn_mask_boundary_iou_counts_u8(const unsigned char *a, int Da, const int32_t *a_label, const unsigned char *b, int Db,
                                      const int32_t *b_label, int H, int W, int dilation, void *ws, size_t ws_bytes, int32_t *inter,
                                      int32_t *area_a, int32_t *area_b, int32_t *binter, int32_t *barea_a, int32_t *barea_b,
                                      void *stream);

/* ------------------------------------------------------------------------------------------
 * Keypoint heat-map decode (keypoints.hip; MaskRCNN.predict_keypoints).  Replaces the host NumPy of the reference's viewer.py:86-107
 * (argmax over the cells of predict()'s (D, K, S*S) heat maps, maskrcnn.py:247-251, mapped into the box).
 *   heat (D,S,S,Cp) float32 NHWC, 16-byte aligned, Cp % 4 == 0, Cp >= K: the keypoint branch's output; channels k >= K are not used
 *   bbox (D,4) float32 (y1,x1,y2,x2) in image coordinates
 *   out (D,K,4) float32, 16-byte aligned: (y, x, logit, prob) of the maximum of channel k over the S*S cells, where
 *     idx   = the FIRST flat index cy * S + cx of the maximum (np.argmax's tie-break; finite inputs)
 *     y     = float(idx / S) * ((y2 - y1) / S) + y1,  x = float(idx % S) * ((x2 - x1) / S) + x1  (float32, no FMA: the cell's
 *             top-left corner, the viewer's rule and the inverse of the training target's floor((kp - y0) / h * S))
 *     logit = the maximum value (bit-exact), prob = 1 / sum_cells exp(l - logit) (the softmax over the cells, at the argmax)
 *   index (D,K) int32 or NULL: idx
 *   ws: device scratch of mrcnn_keypoint_decode_workspace_bytes(D, S, K) bytes (per-split partial reductions)
 * Bit-identical from run to run.  D == 0 is a no-op.  Errors, before any launch: MRCNN_E_INVALID for bad sizes, Cp not a multiple
 * of 4, a NULL or misaligned heat / out, a NULL bbox; MRCNN_E_UNSUPPORTED for K > 256 or S > 46340; MRCNN_E_WORKSPACE for a short
 * or NULL workspace.
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_keypoint_decode_workspace_bytes(int D, int S, int K);
int mrcnn_keypoint_decode_f32(const float *heat, int D, int S, int Cp, int K, const float *bbox, void *ws, size_t ws_bytes, float *out,
                              int32_t *index, void *stream);

/* ------------------------------------------------------------------------------------------
 * COCO run-length encoding of masks (rle.hip; InstanceSegmentationCOCOEvaluator, evaluate.py).  Replaces pycocotools' maskApi.c rleEncode
 * on host copies of the masks.
 *   m (D,H,W) uint8, contiguous rows (no alignment needed); any nonzero byte is a set pixel (torch.bool, mask_paste)
 *   runs over the column-major flattening p = x * H + y, alternating 0 / 1 and starting with a run of 0s (a mask whose pixel (0,0) is
 *   set starts with a 0-length run; an all-zero mask is [H * W])
 *   count: offsets (D+1) int32 = exclusive prefix sum of the masks' run counts (offsets[D] = the total); area (D) int32 or NULL = the
 *          set-pixel count of each mask
 *   write: counts[offsets[d] .. offsets[d+1]) = the runs of mask d; ws must be the workspace count used, unmodified (it holds the
 *          per-segment ranks count computed), and offsets count's output
 *   ws: device scratch of mrcnn_mask_rle_workspace_bytes(D, H, W) bytes
 * Exact integers, identical from run to run and independent of the launch split.  D == 0 is valid (count writes offsets[0] = 0).
 * Errors, before any launch: MRCNN_E_INVALID for a negative size or a NULL pointer of a non-empty side; MRCNN_E_WORKSPACE for a short
 * workspace; MRCNN_E_UNSUPPORTED when H * W or the worst-case run total D * (H * W + 1) does not fit int32.
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_mask_rle_workspace_bytes(int D, int H, int W);
int mrcnn_mask_rle_count_u8(const unsigned char *m, int D, int H, int W, void *ws, size_t ws_bytes, int32_t *offsets, int32_t *area,
                            void *stream);
int mrcnn_mask_rle_write_u8(const unsigned char *m, int D, int H, int W, const void *ws, size_t ws_bytes, const int32_t *offsets,
                            int32_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------
 * Batched training resizes with an optional horizontal flip (augment.hip; dataset/loader.py BatchLoader(augment=...)).  The device
 * side of Transform(hflip(example)) for a whole batch: every raw example of the batch is packed into one uint8 buffer and resized,
 * mirrored or not, straight into the zero-padded batch tensor in ONE launch per tensor, padding included (no memset).
 *   desc (N) HOST array, read at the call (passed to the kernel by value): per example
 *     src_offset  byte offset of the example's source in src (image: (H,W,3) HWC; masks: (count,H,W))
 *     H, W        source size;  oh, ow  resized size (oh <= dst_h, ow <= dst_w);  flip  0 or 1: source column s is read as W-1-s
 *     count       masks: instances of the example (<= G; rows [count, G) are written zero); images: ignored
 *   src_bytes   size of src: every example's source must lie inside it
 *   image: dst (N,3,dst_h,dst_w) float32, 16-byte aligned: dst[n,c,y,x] = resize_linear(src_n[..., ::-1] if flip else src_n)[c,y,x] / div
 *          for y < oh, x < ow (the taps of mrcnn_image_resize_u8_f32, bit-identical), 0 elsewhere
 *   masks: dst (N,G,dst_h,dst_w) uint8, 16-byte aligned: resize_nearest(mask[:, ::-1] if flip else mask) for g < count, y < oh, x < ow
 *          (the rule of mrcnn_mask_resize_nearest_u8), 0 elsewhere
 * Errors, before any launch: MRCNN_E_INVALID for N outside 1..MRCNN_RESIZE_BATCH_MAX, bad sizes, a flip other than 0 / 1, a count
 * outside 0..G, a source outside src_bytes, a NULL desc / dst, a NULL src with a non-empty source, a misaligned dst.
 * ---------------------------------------------------------------------------------------- */
#define MRCNN_RESIZE_BATCH_MAX 32
typedef struct mrcnn_resize_desc {
    long long src_offset;
    int H, W, oh, ow, flip, count;
} mrcnn_resize_desc_t;          /* 32 bytes */
int mrcnn_image_resize_batch_u8_f32(const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, float *dst,
                                    int dst_h, int dst_w, float div, void *stream);
int mrcnn_mask_resize_batch_nearest_u8(const unsigned char *src, size_t src_bytes, const mrcnn_resize_desc_t *desc, int N, int G,
                                       unsigned char *dst, int dst_h, int dst_w, void *stream);

/* ------------------------------------------------------------------------------------------
 * Large-scale jitter (augment.hip; dataset/augment.py lsj_geometry): the batched resizes above with a crop window.  The
 * example is resized VIRTUALLY to oh x ow (either may exceed the canvas) and the window of rows y0 .. y0+ch-1, columns x0 .. x0+cw-1 of
 * that resize lands at the top-left of the dst_h x dst_w canvas: output (y, x), y < ch, x < cw, is what the kernels above give at
 * (y + y0, x + x0) of an oh x ow resize (same taps, flip = mirrored source column), everything else in the canvas is zero.
 *   mrcnn_image_resize_crop_batch_u8_f32     the image writer: dst (N,3,dst_h,dst_w) float32.  One launch.
 *   mrcnn_mask_crop_boxes_u8                 what the crop leaves of each instance, without writing a plane: src holds each example's
 *       (count,H,W) masks, count <= Gin; labels_in (N,Gin) int32.  An instance is KEPT when its cropped nearest-neighbour resize has a
 *       non-zero pixel.  Per example the kept instances, in their order, fill output rows 0, 1, ... (kept instances past row G-1 are
 *       dropped): bboxes (N,G,4) float32 = the tight box (ymin, xmin, ymax + 1, xmax + 1) of the cropped mask in canvas coordinates,
 *       labels (N,G) int32 = the instance's labels_in entry, gather (N,G) int32 = its index among the example's source instances; the
 *       rows behind them are (0,0,0,0), -1, -1.  ws: (N,Gin,4) int32 scratch, 16-byte aligned, filled by the call.  One fill and two
 *       launches on `stream`; integer maxima only - exact, the same for every schedule.
 *   mrcnn_mask_resize_crop_batch_nearest_u8  the mask writer: dst (N,G,dst_h,dst_w) uint8; output plane j of example n reads source
 *       instance gather[n][j] (DEVICE, (N,G) int32); an entry of -1, or outside the example's count, gives a zero plane.  One launch.
 * Errors, before any launch: MRCNN_E_INVALID for everything the calls above refuse (with the window, not oh x ow, held against the
 * canvas), ch > dst_h, cw > dst_w, y0 + ch > oh, x0 + cw > ow, a negative offset, an empty window, a NULL labels_in / bboxes / labels /
 * gather / ws, a misaligned bboxes / ws.
 * ---------------------------------------------------------------------------------------- */
typedef struct mrcnn_crop_desc {
    long long src_offset;
    int H, W, oh, ow, flip, count;
    int y0, x0, ch, cw;
} mrcnn_crop_desc_t;            /* 48 bytes */
int mrcnn_image_resize_crop_batch_u8_f32(const unsigned char *src, size_t src_bytes, const mrcnn_crop_desc_t *desc, int N, float *dst,
                                         int dst_h, int dst_w, float div, void *stream);
int mrcnn_mask_crop_boxes_u8(const unsigned char *src, size_t src_bytes, const mrcnn_crop_desc_t *desc, int N, int Gin, int G, int dst_h,
                             int dst_w, const int32_t *labels_in, float *bboxes, int32_t *labels, int32_t *gather, int32_t *ws,
                             void *stream);
int mrcnn_mask_resize_crop_batch_nearest_u8(const unsigned char *src, size_t src_bytes, const mrcnn_crop_desc_t *desc, int N, int G,
                                            const int32_t *gather, unsigned char *dst, int dst_h, int dst_w, void *stream);

/* ------------------------------------------------------------------------------------------
 * Simple Copy-Paste on a large-scale-jitter batch (copy_paste.hip; dataset/augment.py copy_paste_batch is the rule).
 * Inputs, all DEVICE, the pre-paste batch - nothing is updated in place: imgs (N,3,H,W) float32, masks (N,G,H,W) uint8, labels (N,G)
 * int32 (-1: no instance), gather (N,G) int32 (the ORIGINAL instance index of each row, mrcnn_mask_crop_boxes_u8's table), sel (N,Gin)
 * uint8 (is original instance i of example n offered as a source), receive (N) uint8 (is example n a target).  Example n's partner is
 * p = (n + 1) % N; with receive[n] its rows j with labels[p][j] >= 0, 0 <= gather[p][j] < Gin and sel[p][gather[p][j]] != 0 are pasted.
 *   mrcnn_copy_paste_image_f32  alpha (N,H,W) uint8 = 0xFF where a pasted row of the partner is non-zero, 0 elsewhere;
 *       out_imgs[n] = alpha[n] ? imgs[p] : imgs[n] on the 3 channels.  One launch.
 *   mrcnn_copy_paste_masks_u8   the candidates of example n are its own rows r with labels[n][r] >= 0, as masks[n][r] where alpha[n] is 0,
 *       then the pasted rows of the partner, unchanged.  Those with a pixel left, in that order, fill output rows 0, 1, ... (those past row
 *       G_out - 1 are dropped): out_masks (N,G_out,H,W) uint8, bboxes (N,G_out,4) float32 = the tight box (ymin, xmin, ymax + 1, xmax + 1),
 *       labels_out (N,G_out) int32, source (N,G_out) int32 = r for an own row, G + j for a partner row; the rows behind them are a zero
 *       plane, (0,0,0,0), -1, -1.  alpha: the plane of mrcnn_copy_paste_image_f32 for the same inputs.  ws: (N,2G,4) int32 scratch, filled
 *       by the call.  One fill and three launches on `stream`; integer maxima only - exact, the same for every schedule.
 * Errors, before any launch: MRCNN_E_INVALID for a NULL pointer, N outside 2..MRCNN_RESIZE_BATCH_MAX, G / Gin / G_out outside 1..65535,
 * H or W not positive or H * (W + 15) past INT_MAX, out_imgs / alpha / out_masks / bboxes / ws not 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_copy_paste_image_f32(const float *imgs, const unsigned char *masks, const int32_t *labels, const int32_t *gather,
                               const unsigned char *sel, const unsigned char *receive, int N, int G, int Gin, int H, int W,
                               float *out_imgs, unsigned char *alpha, void *stream);
int mrcnn_copy_paste_masks_u8(const unsigned char *masks, const unsigned char *alpha, const int32_t *labels, const int32_t *gather,
                              const unsigned char *sel, const unsigned char *receive, int N, int G, int Gin, int G_out, int H, int W,
                              unsigned char *out_masks, float *bboxes, int32_t *labels_out, int32_t *source, int32_t *ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * Test-time augmentation (tta.hip; MaskRCNN.use_test_augmentation).  An image runs as V <= MRCNN_TTA_VIEWS_MAX views (short sides,
 * optionally mirrored), one N = 1 forward each; these calls merge the views after the forward pass.
 *   views (V) HOST array, read at the call (passed to the kernels by value): R = the view's candidates (decode), mirror 0 / 1, scale = the
 *         view's resize factor ow / W (decode).  The merges read mirror only.
 *   *const *: V HOST-side device pointers, one per view (the precedent of mrcnn_roi_align_fpn_fwd_f32's xs)
 * image_resize_mirror: mrcnn_image_resize_f32 with mirror = 1 reading source column s as W-1-s: bit-identical to resizing img[..., ::-1].
 * tta_detect_decode: the rows of all views concatenated in view order into cls_bbox (R,4) / prob (R,n_class), R = sum of views[v].R;
 *   row i of view v = mrcnn_detect_decode_f32 of rois[v][i], box_out[v][i] with views[v].scale and the original (size_h, size_w);
 *   a mirrored view's box is then mapped to (y1, size_w - x2, y2, size_w - x1).  rois[v] / box_out[v] may be NULL when R = 0.
 * class_nms_ws: mrcnn_class_nms_f32 for R <= MRCNN_CLASS_NMS_WS_MAX candidates (same outputs, same keep lists), no host sync.
 *   R <= 512 runs mrcnn_class_nms_f32 itself (ws unused, may be NULL); above, ws of mrcnn_class_nms_workspace_bytes(R, n_class) bytes,
 *   256-byte aligned (the sorted candidates and the IoU bitmask of every class).  R > MRCNN_CLASS_NMS_WS_MAX: MRCNN_E_UNSUPPORTED.
 * tta_mask_merge: prob (D,S,S) = (sum over views u, in order, of sigmoid(mask_logits[u][d, y, x_u, label[d]])) / V, float32,
 *   x_u = S-1-x for a mirrored view; mask_logits[u] (D,S,S,Cm) NHWC as mrcnn_mask_paste_f32 takes them.
 * mask_paste_prob: mrcnn_mask_paste_f32 from probabilities prob (D,S,S) instead of logits (bbox (D,4) 16-byte aligned).
 * tta_keypoint_merge: out (D,S,S,Cp) = (sum over views u, in order, of heat[u][d, y, x_u, k_u]) / V, x_u as above, k_u = perm[k] for a
 *   mirrored view and k < K, k otherwise.  perm: HOST array of K ints (a permutation of 0..K-1), needed when a view is mirrored.
 * D == 0 and R == 0 are no-ops.  Errors, before any launch: MRCNN_E_INVALID for V outside 1..MRCNN_TTA_VIEWS_MAX, a mirror other than
 * 0 / 1, bad sizes or scales, NULL pointers, a bad permutation, a misaligned workspace; MRCNN_E_WORKSPACE for a short or NULL workspace;
 * MRCNN_E_UNSUPPORTED for R > MRCNN_CLASS_NMS_WS_MAX or K > MRCNN_TTA_KEYPOINTS_MAX.
 * ---------------------------------------------------------------------------------------- */
#define MRCNN_TTA_VIEWS_MAX 8
#define MRCNN_TTA_KEYPOINTS_MAX 256
#define MRCNN_CLASS_NMS_WS_MAX 4096
typedef struct mrcnn_tta_view {
    int R, mirror;
    float scale;
} mrcnn_tta_view_t;             /* 12 bytes */
int mrcnn_image_resize_mirror_f32(const float *src, int C, int H, int W, float *dst, int oh, int ow, int dst_h, int dst_w, int mirror,
                                  float div, void *stream);
int mrcnn_tta_detect_decode_f32(const float *const *rois, const float *const *box_out, const mrcnn_tta_view_t *views, int V, int ld,
                                int n_class, int loc0, const float *loc_mean4, const float *loc_std4, float size_h, float size_w,
                                float *cls_bbox, float *prob, void *stream);
size_t mrcnn_class_nms_workspace_bytes(int R, int n_class);
int mrcnn_class_nms_ws_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end, float score_thresh,
                           float nms_thresh, int32_t *keep_idx, int32_t *keep_cnt, void *ws, size_t ws_bytes, void *stream);
int mrcnn_tta_mask_merge_f32(const float *const *mask_logits, const mrcnn_tta_view_t *views, int V, int D, int S, int Cm,
                             const int32_t *label, float *prob, void *stream);
int mrcnn_mask_paste_prob_f32(const float *prob, int D, int S, const float *bbox, int H, int W, unsigned char *out, void *stream);
int mrcnn_tta_keypoint_merge_f32(const float *const *heat, const mrcnn_tta_view_t *views, int V, int D, int S, int Cp, int K,
                                 const int32_t *perm, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Frozen BatchNorm in the training step (bn_frozen.hip; MaskRCNN.freeze).  A frozen layer is mrcnn_bn_infer_fwd_f32 inside the
 * training step: gamma, beta, avg_mean, avg_var are constants, nothing is reduced, no workspace.  float32, NHWC (P rows of C
 * channels), C % 4 == 0, every pointer 16-byte aligned.  With a[c] = gamma[c] * (1.0f / sqrtf(avg_var[c] + eps)):
 * bn_frozen_bwd: dz = gy under the ReLU mask, gx = dz * a[c], gres (nullable, a buffer of its own) = dz.  relu: 0 no mask (also a gy
 *   that arrives masked), 1 mask = (yx > 0) with yx the layer's output y, 2 mask recomputed from yx = the layer's input x by the
 *   forward's expression gamma * ((x - avg_mean) * (1.0f / sqrtf(avg_var + eps))) + beta > 0 (BatchNorm + ReLU without a residual).
 *   yx may be NULL for relu 0, beta / avg_mean for relu 0 and 1.  gx may be gy.
 * bn_infer_fwd_pair: y = relu(bn_a(xa) + bn_b(xb)), the bits of mrcnn_bn_infer_fwd_f32(xb) followed by
 *   mrcnn_bn_infer_fwd_f32(xa, residual = that, relu = 1) without the intermediate tensor.
 * bn_frozen_bwd_pair: dz = y ? gy where y > 0 : gy (y NULL: gy arrives masked); gxa = dz * a_a[c], gxb = dz * a_b[c]: the bits of
 *   two bn_frozen_bwd calls.  gxa or gxb may be gy; gxa != gxb.
 * sgd_momentum_wd_masked: mrcnn_sgd_momentum_wd_f32 over n elements starting at element `offset` of the flat parameter buffer
 *   (p, g, v point AT that element; the flat buffers are 16-byte aligned), skipping every 64-float block b of the flat buffer whose bit
 *   (frozen_blocks[b / 32] >> (b % 32)) & 1 is set: such elements of p and v are neither read nor written.  n_blocks = blocks the mask
 *   covers (>= ceil((offset + n) / 64)).  Trainable elements get the bits of the unmasked call.  n == 0 is a no-op.
 * Errors, before any launch: MRCNN_E_INVALID for a NULL or misaligned pointer, P <= 0, C % 4 != 0, a relu outside 0..2, an aliased
 * output that may not alias, a section outside the mask.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_bn_frozen_bwd_f32(const float *gy, const float *yx, const float *gamma, const float *beta, const float *avg_mean,
                            const float *avg_var, float *gx, float *gres, int P, int C, float eps, int relu, void *stream);
int mrcnn_bn_infer_fwd_pair_f32(const float *xa, const float *gamma_a, const float *beta_a, const float *mean_a, const float *var_a,
                                const float *xb, const float *gamma_b, const float *beta_b, const float *mean_b, const float *var_b,
                                float *y, int P, int C, float eps, void *stream);
int mrcnn_bn_frozen_bwd_pair_f32(const float *gy, const float *y, const float *gamma_a, const float *var_a, const float *gamma_b,
                                 const float *var_b, float *gxa, float *gxb, int P, int C, float eps, void *stream);
int mrcnn_sgd_momentum_wd_masked_f32(float *p, const float *g, float *v, size_t n, size_t offset, const uint32_t *frozen_blocks,
                                     size_t n_blocks, float lr, float momentum, float weight_decay, void *stream);

/* ------------------------------------------------------------------------------------------
 * Gradient accumulation, gradient-norm clipping and the update with a device-resident learning rate (optim.hip).  float32 streaming
 * kernels over sections of the flat buffers, addressed like mrcnn_sgd_momentum_wd_masked_f32: n elements starting at element `offset`
 * of the flat buffer, every data pointer points AT that element of a 16-byte aligned flat buffer; frozen_blocks is that function's
 * mask (n_blocks >= ceil((offset + n) / 64)) or NULL = nothing frozen (n_blocks is then ignored); elements of frozen blocks are neither
 * read nor written.  No host synchronisation, no atomics; the same input gives the same bits on every run.
 *
 * The hyper block is MRCNN_HYPER_FLOATS floats of device memory owned by the caller:
 *   [MRCNN_HYPER_LR] learning rate, [MRCNN_HYPER_A] a = 1 or 1 / (number of micro-batches), [MRCNN_HYPER_THRESHOLD] clip threshold
 *   (+inf: never clip) - placed by the caller; [MRCNN_HYPER_SCALE], [MRCNN_HYPER_NORM], [MRCNN_HYPER_RATE] - written by grad_norm_hyper
 *   (a caller that takes no norm places scale = a itself); [MRCNN_HYPER_SKIPPED] a uint32 counter of skipped updates.
 *
 * grad_accumulate: acc = g (first != 0) or acc = acc + g.  acc != g.
 * grad_norm_hyper: S = sum of (acc + g)^2 (acc NULL: g^2) over the trainable elements, every square and every partial sum in double,
 *   combined in a fixed order (per-block partials in `workspace`, mrcnn_grad_norm_workspace_bytes(n) bytes, 8-byte aligned); then, on
 *   the device, norm = (float)sqrt(S) * a; rate = norm > threshold ? threshold / norm : 1.0f; scale = a * rate.  A non-finite norm gives
 *   rate = scale = 0 and increments the skipped counter.  The norm is taken over ONE section: pass the whole buffer.
 * sgd_momentum_wd_hyper: ge = acc + g (acc NULL: g); gs = ge * scale; v = momentum * v - lr * (gs + wd * p); p += v, with lr and scale
 *   read from the hyper block.  scale == 0 takes gs = 0 whatever ge holds (a skipped update: inf * 0 would be nan).  With scale == 1.0f
 *   and acc NULL the bits of mrcnn_sgd_momentum_wd_f32 / _masked_f32.  n == 0 is a no-op (also for grad_accumulate).
 * Errors, before any launch: MRCNN_E_INVALID for a NULL or misaligned pointer, a section outside the mask, a workspace too small.
 * ---------------------------------------------------------------------------------------- */
#define MRCNN_HYPER_FLOATS 8
#define MRCNN_HYPER_LR 0
#define MRCNN_HYPER_A 1
#define MRCNN_HYPER_THRESHOLD 2
#define MRCNN_HYPER_SCALE 3
#define MRCNN_HYPER_NORM 4
#define MRCNN_HYPER_RATE 5
#define MRCNN_HYPER_SKIPPED 6
int mrcnn_grad_accumulate_f32(float *acc, const float *g, size_t n, size_t offset, const uint32_t *frozen_blocks, size_t n_blocks,
                              int first, void *stream);
size_t mrcnn_grad_norm_workspace_bytes(size_t n);
int mrcnn_grad_norm_hyper_f32(const float *acc, const float *g, size_t n, size_t offset, const uint32_t *frozen_blocks, size_t n_blocks,
                              float *hyper, void *workspace, size_t workspace_bytes, void *stream);
int mrcnn_sgd_momentum_wd_hyper_f32(float *p, const float *acc, const float *g, float *v, size_t n, size_t offset,
                                    const uint32_t *frozen_blocks, size_t n_blocks, const float *hyper, float momentum, float weight_decay,
                                    void *stream);

/* ------------------------------------------------------------------------------------------
 * Rendering of detections (vis.hip; chainer_maskrcnn/vis.py, demo.py).  One launch turns an image and its
 * detections into a picture on the device; integer arithmetic only, the same bytes on every run.
 *   img (3,H,W) float32 RGB, values 0..255 as predict takes it; out (H,W,3) uint8 RGB, contiguous.
 *   masks (D,H,W) bytes, any nonzero byte is a set pixel (rows may start at any byte offset); bbox (D,4) float32 (y1,x1,y2,x2);
 *   colors (D,3) uint8; prims: n_prims descriptors in DEVICE memory, 16-byte aligned; font: n_glyphs uint64 in DEVICE memory, bit
 *   5 * row + col of font[g] = pixel (row, col) of the 5 x 7 glyph g.
 * Per pixel, painter's order:
 *   c = min(255, max(0, floor(v + 0.5))) per channel (float32 arithmetic; NaN gives 0);
 *   for d = order[0], .., order[D-1] (order: D int32 in DEVICE memory; NULL: d = 0..D-1; an index outside 0..D-1 draws nothing):
 *                   MRCNN_VIS_DRAW_MASKS and mask[d] set: c = blend(c, colors[d], mask_a256);
 *                   MRCNN_VIS_DRAW_CONTOURS and the pixel is set with a 4-neighbour that is unset or outside the image: c = colors[d];
 *                   MRCNN_VIS_DRAW_BOXES and the pixel is on the outline (box_thickness) of the rectangle with the inclusive corners
 *                   (top, left, bottom, right) = floor(bbox[d] + 0.5), each clamped to the coordinate range (NaN: its lower end):
 *                   c = colors[d];
 *   for every primitive in array order: the pixel is on it: c = blend(c, its rgb, its a).
 *   blend(c, col, a) = (c * (256 - a) + col * a + 128) >> 8 per channel, a = round(alpha * 256) in [0, 256].
 * Primitives (all fields int32; rgb = r | g << 8 | b << 16):
 *   MRCNN_VIS_RECT     outline of the rectangle with inclusive corners (x0,y0)-(x1,y1), thickness p >= 1 growing inwards: a pixel of
 *                      the rectangle with x < x0 + p or x > x1 - p or y < y0 + p or y > y1 - p;
 *   MRCNN_VIS_SEGMENT  a = (x0,y0), b = (x1,y1), thickness p; with d = b - a, L = d.d, w = pixel - a, s = w.d, in int64:
 *                      L == 0 or s <= 0: 4 |w|^2 <= p^2;  s >= L: 4 |pixel - b|^2 <= p^2;  otherwise 4 cross(w,d)^2 <= p^2 L;
 *   MRCNN_VIS_DISC     |pixel - (x0,y0)|^2 <= p^2;
 *   MRCNN_VIS_GLYPH    glyph x1 at scale p (1..MRCNN_VIS_GLYPH_SCALE_MAX), top-left (x0,y0): pixel (x,y) of the 5p x 7p cell is on
 *                      when bit 5 * ((y - y0) / p) + (x - x0) / p of font[x1] is set; x1 outside 0..n_glyphs-1: the whole cell;
 *   MRCNN_VIS_FILL     every pixel of the rectangle with inclusive corners (x0,y0)-(x1,y1).
 * Everything is clipped to the image.  Caps: H, W <= MRCNN_VIS_MAX_SIDE; primitive coordinates and rounded box corners within
 * MRCNN_VIS_COORD_MIN..MRCNN_VIS_COORD_MAX (the image and a margin of 4096 around it); p <= MRCNN_VIS_PARAM_MAX; a in 0..256.  With
 * these no term of the segment rule exceeds 2^63.  A primitive that breaks a cap or has an unknown kind draws nothing (the host layer
 * refuses it before the call).  D == 0, n_prims == 0 are valid; H * W == 0 is a no-op.  masks may be NULL when neither masks nor
 * contours are drawn, bbox when boxes are not.
 * Errors, before any launch: MRCNN_E_INVALID for H or W outside 0..MRCNN_VIS_MAX_SIDE, a negative D or n_prims, n_glyphs outside
 * 0..MRCNN_VIS_GLYPHS_MAX, unknown flags, mask_a256 outside 0..256, box_thickness outside 1..MRCNN_VIS_PARAM_MAX, a NULL or
 * misaligned pointer of a side that is used.
 * ---------------------------------------------------------------------------------------- */
#define MRCNN_VIS_MAX_SIDE 16384
#define MRCNN_VIS_COORD_MIN (-4096)
#define MRCNN_VIS_COORD_MAX 20479
#define MRCNN_VIS_PARAM_MAX 4096
#define MRCNN_VIS_GLYPH_W 5
#define MRCNN_VIS_GLYPH_H 7
#define MRCNN_VIS_GLYPH_SCALE_MAX 64
#define MRCNN_VIS_GLYPHS_MAX 256
#define MRCNN_VIS_DRAW_MASKS 1
#define MRCNN_VIS_DRAW_CONTOURS 2
#define MRCNN_VIS_DRAW_BOXES 4
#define MRCNN_VIS_RECT 0
#define MRCNN_VIS_SEGMENT 1
#define MRCNN_VIS_DISC 2
#define MRCNN_VIS_GLYPH 3
#define MRCNN_VIS_FILL 4
typedef struct mrcnn_vis_prim {
    int32_t kind, x0, y0, x1, y1, p, rgb, a;
} mrcnn_vis_prim_t;             /* 32 bytes */
int mrcnn_vis_render_u8(const float *img, int H, int W, const unsigned char *masks, const float *bbox, const unsigned char *colors,
                        const int32_t *order, int D, int mask_a256, int box_thickness, int flags, const mrcnn_vis_prim_t *prims, int n_prims,
                        const unsigned long long *font, int n_glyphs, unsigned char *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Soft-NMS and box voting (boxpost.hip; MaskRCNN.use_soft_nms / use_box_voting).  Detectron's TEST.SOFT_NMS and
 * TEST.BBOX_VOTE on the outputs of mrcnn_detect_decode_f32 / mrcnn_tta_detect_decode_f32: cls_bbox (R,4), prob (R,n_class), classes
 * l in [l_begin, l_end), float32 throughout, no contraction, correctly rounded divisions.  iou(b, c) = ai / ((area_b + area_c) - ai), the
 * expression of mrcnn_class_nms_f32.  A row i is a candidate of class l when prob[i,l] > score_thresh.
 * class_soft_nms: per class, with the working scores s_i = prob[i,l] of its candidates: while a candidate remains, take m = the largest
 *   (s, i) (score descending, then index descending); keep_idx[l][cnt] = m, keep_score[l][cnt] = s_m; remove m; every remaining c gets
 *   s_c = s_c * w(iou(box_m, box_c)) and is removed unless s_c > score_thresh.  w by method: MRCNN_SOFT_NMS_HARD 0 at iou >= nms_thresh
 *   (the keep lists of mrcnn_class_nms_f32, scores unchanged); MRCNN_SOFT_NMS_LINEAR 1 - iou at iou >= nms_thresh; MRCNN_SOFT_NMS_GAUSSIAN
 *   expf(-(iou * iou) / sigma) at iou > 0; 1 otherwise (a NaN iou included).  keep_idx (n_class,R) int32, keep_score (n_class,R) float32,
 *   keep_cnt (n_class) int32 (0 outside [l_begin, l_end)); rows >= keep_cnt[l] are left unwritten.  0 < R <= MRCNN_BOXPOST_MAX.  A class
 *   with up to MRCNN_SOFT_NMS_LDS_MAX candidates runs in LDS; R above that needs ws of mrcnn_class_soft_nms_workspace_bytes(R, n_class)
 *   bytes, 16-byte aligned (otherwise ws is unused and may be NULL).  One launch, no host synchronisation.
 * box_vote: for every kept detection k < keep_cnt[l] of class l, with b = cls_bbox[keep_idx[l][k]]: over the candidates c of the class with
 *   iou(b, box_c) >= vote_thresh, keep_box[l][k] = (sum of prob[c,l] * box_c) / (sum of prob[c,l]) per coordinate (Detectron's scoring
 *   method ID: scores are not changed); b itself when no candidate qualifies (a zero-area b).  Fixed summation order, no atomics: the
 *   same bits on every run.  keep_box (n_class,R,4) float32, 16-byte aligned; rows >= keep_cnt[l] are left unwritten.
 * Errors, before any launch: MRCNN_E_INVALID for a NULL pointer, R <= 0, n_class <= 0, an l range outside [0, n_class], an unknown
 * method, sigma <= 0, a vote_thresh outside (0, 1], a negative score_thresh of box_vote (its weights must be positive), a misaligned
 * pointer; MRCNN_E_UNSUPPORTED for R > MRCNN_BOXPOST_MAX; MRCNN_E_WORKSPACE
 * for a short or NULL workspace.
 * ---------------------------------------------------------------------------------------- */
#define MRCNN_BOXPOST_MAX 4096
#define MRCNN_SOFT_NMS_LDS_MAX 2048
#define MRCNN_SOFT_NMS_HARD 0
#define MRCNN_SOFT_NMS_LINEAR 1
#define MRCNN_SOFT_NMS_GAUSSIAN 2
size_t mrcnn_class_soft_nms_workspace_bytes(int R, int n_class);
int mrcnn_class_soft_nms_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end, float score_thresh,
                             int method, float nms_thresh, float sigma, int32_t *keep_idx, float *keep_score, int32_t *keep_cnt,
                             void *ws, size_t ws_bytes, void *stream);
int mrcnn_box_vote_f32(const float *cls_bbox, const float *prob, int R, int n_class, int l_begin, int l_end, float score_thresh,
                       float vote_thresh, const int32_t *keep_idx, const int32_t *keep_cnt, float *keep_box, void *stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm of the RoI heads (groupnorm.hip, gn_common.h; nn/core.py GroupNorm).  float32, NHWC (R,H,W,Cp): C logical
 * channels zero-padded to Cp, G groups of cpg = C / G channels, statistics per (sample r, group g) over n = H * W * cpg elements:
 *   mean = sum(x) / n, var = sum((x - mean)^2) / n (biased, taken about the mean: no E[x^2] - E[x]^2), rstd = 1.0f / sqrtf(var + eps).
 * group_norm_fwd: y = gamma[c] * ((x - mean) * rstd) + beta[c], relu != 0: max(y, 0).  Channels c >= C of y are written as exact zeros.
 *   mean, rstd (R,G): written when not NULL (training); each may be NULL.
 * group_norm_bwd: with xh = (x - mean) * rstd, dz = gy (relu 0: also a gy that arrives masked) or gy where the forward's
 *   gamma * xh + beta > 0, else 0 (relu 1: the mask recomputed from x, the bits of the forward's y > 0), gt = dz * gamma:
 *   gx = rstd * (gt - sum_g(gt) / n - xh * (sum_g(gt * xh) / n)), the sums over the group of the sample; channels c >= C as exact zeros.
 *   ggamma[c] = sum over r, h, w of dz * xh, gbeta[c] = sum of dz, (Cp) each, written (accumulate_params 0) or added to what is there
 *   (1); channels c >= C receive 0.  ws: the per-sample partial rows, bwd_ws_bytes of the plan query, summed over r in a fixed order:
 *   no float atomics, the same input gives the same bits on every run.
 * group_norm_plan: host arithmetic only.  path (nullable): 0 = the register-resident kernels (cpg 1, 2 or a multiple of 4 up to 256, and
 *   H * W up to 8 * (256 / cols) with cols = 8 float4 columns per workgroup where cpg divides 32, else cpg / 4: 256 pixels for the head's
 *   cpg 8), which read x (and gy) once; 1 = the generic kernels, which re-read them.  bwd_ws_bytes (nullable) = 2 * R * Cp * 4.
 * x, y, gy, gx, gamma, beta, ggamma, gbeta and ws 16-byte aligned.  R == 0 succeeds without a launch.  Errors, before any launch:
 * MRCNN_E_INVALID for G not dividing C, Cp < C, Cp % 4 != 0, a non-positive H, W, C, G or eps, a negative R, H * W * Cp above 2^31 - 1,
 * a relu outside 0..1, a NULL or misaligned pointer, a workspace too small.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_group_norm_plan(int R, int H, int W, int C, int Cp, int G, int *path, size_t *bwd_ws_bytes);
int mrcnn_group_norm_fwd_f32(const float *x, const float *gamma, const float *beta, int R, int H, int W, int C, int Cp, int G, float eps,
                             int relu, float *y, float *mean, float *rstd, void *stream);
int mrcnn_group_norm_bwd_f32(const float *gy, const float *x, const float *gamma, const float *beta, const float *mean, const float *rstd,
                             int R, int H, int W, int C, int Cp, int G, int relu, float *gx, float *ggamma, float *gbeta,
                             int accumulate_params, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm of whole feature maps (groupnorm_map.hip, gn_common.h; nn/core.py MapGroupNorm).  The tensors, the
 * channel geometry, y, gx, ggamma and gbeta of group_norm_* above without its relu, for maps too large for one workgroup per (sample,
 * group): a sample is cut into `chunks` contiguous ranges of pixels_per_chunk pixels (the last may be shorter), one workgroup per (sample,
 * chunk) over all channels, and every hand-over between workgroups is a kernel boundary - three launches forward, three backward, no
 * atomics, no counters: the same input gives the same bits on every run.
 *   statistics: each chunk i states, per group, its own mean m_i over its n_i elements and M2_i = sum((x - m_i)^2); they are merged in
 *   chunk order by  d = m_i - m, m += d * n_i / (n + n_i), M2 += M2_i + d * d * n * n_i / (n + n_i);  mean = m,
 *   rstd = 1.0f / sqrtf(M2 / n + eps) (a variance about a mean: no E[x^2] - E[x]^2).  mean, rstd (R,G): written when not NULL.
 * group_norm_map_plan: host arithmetic only; every output is nullable.  pixels_per_chunk and chunks are functions of H * W and Cp alone
 *   (chunks * pixels_per_chunk >= H * W > (chunks - 1) * pixels_per_chunk); fwd_ws_bytes = (2 * R * chunks * G + 2 * R * G) * 4,
 *   bwd_ws_bytes = (2 * R * chunks * Cp + 2 * R * G) * 4.
 * The map path takes cpg = C / G a multiple of 4 up to 256 (a float4 stays inside one group) and Cp up to 1024; every other geometry is
 *   MRCNN_E_INVALID from all three calls - group_norm_* serves it.
 * x, y, gy, gx, gamma, beta, ggamma, gbeta and ws 16-byte aligned.  R == 0 succeeds without a launch.  Errors, before any launch:
 * MRCNN_E_INVALID for G not dividing C, Cp < C, Cp % 4 != 0, a non-positive H, W, C, G or eps, a negative R, H * W * Cp above 2^31 - 1,
 * a NULL or misaligned pointer, a workspace too small.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_group_norm_map_plan(int R, int H, int W, int C, int Cp, int G, int *pixels_per_chunk, int *chunks, size_t *fwd_ws_bytes,
                              size_t *bwd_ws_bytes);
int mrcnn_group_norm_map_fwd_f32(const float *x, const float *gamma, const float *beta, int R, int H, int W, int C, int Cp, int G, float eps,
                                 float *y, float *mean, float *rstd, void *ws, size_t ws_bytes, void *stream);
int mrcnn_group_norm_map_bwd_f32(const float *gy, const float *x, const float *gamma, const float *mean, const float *rstd, int R, int H, int W,
                                 int C, int Cp, int G, float *gx, float *ggamma, float *gbeta, int accumulate_params, void *ws,
                                 size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Cascade R-CNN box stages (cascade.hip, box_common.h; no counterpart in the reference).  float32, no contraction,
 * correctly rounded divisions.
 * cascade_refine: stage k -> stage k+1 over the R = N * S rows of the sampler's fixed row block (image i owns rows [i * S, (i + 1) * S)),
 *   one launch, grid (ceil(S / 256), N), no host synchronisation.
 *   rois (R,4) (y1,x1,y2,x2): stage k's input boxes in the forward's frame; box_out (R,ld): stage k's output, its class-agnostic deltas in
 *   columns loc0 .. loc0 + 3; prev_label (R) int32, nullable: rows with a label < 0 pass through as padding (zero box, level 0, label -1).
 *   mean4, std_prev4, std_next4: HOST arrays of 4 floats, read during the call.  per_image_hw: (N,2) device floats (h, w) of each image, or
 *   NULL = every image is img_h x img_w.
 *   Decode: d = box_out * std_prev + mean, loc2bbox as mrcnn_detect_decode_f32 without the un-scale, every corner clipped
 *   fmaxf(fminf(v, lim), 0); no clamp on dh / dw (an overflowing expf clips to the full extent, the box is always finite).  levels = the
 *   level map of mrcnn_map_rois_to_fpn_levels_f32 (k_min 0, k_max 4) of the refined box; rois_xy5 = (i, x1, y1, x2, y2).
 *   gt_boxes (N,gt_cap,4), nullable: NULL = inference, only roi, rois_xy5 and levels are written and gt_labels, n_gt, std_next4, gt_loc,
 *   label, gt_assign must be NULL too.  Otherwise the refined box is matched against the image's first min(n_gt[i], gt_cap) boxes with the IoU
 *   and the NumPy max / argmax of mrcnn_proposal_target_f32 (first maximum; a NaN wins, the first NaN stays):
 *     empty refined box (a side <= 0 after clipping): label -1, assign -1, gt_loc 0 (ignored by both losses; box and level still written)
 *     no ground truth in the image: label 0, assign -1, gt_loc 0
 *     else assign = argmax, label = gt_labels[argmax] + 1 where max >= iou_thresh (a NaN maximum: background), else 0;
 *     gt_loc = (bbox2loc(roi, gt[argmax]) - mean) / std_next where label > 0, zeros elsewhere.
 *   N == 0 or S == 0 succeeds without a launch.  Errors, before any launch: MRCNN_E_INVALID for a NULL rois / box_out / roi / rois_xy5 /
 *   levels / mean4 / std_prev4, ld < loc0 + 4, negative sizes, N > 65535, ground-truth arguments that do not come together;
 *   MRCNN_E_UNSUPPORTED for gt_cap > 256.
 * cascade_prob: prob (R,n_class) = the mean over the K stages (2 <= K <= 4; box_out0 .. box_out{K-1}, the rest NULL; all (R,ld)) of the
 *   softmax of columns 0 .. n_class - 1, each softmax with the arithmetic of mrcnn_detect_decode_f32, added in stage order and divided by
 *   (float)K: ((p1 + p2) + p3) / 3.  One launch, one wave per row.  R == 0 succeeds without a launch.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_cascade_refine_f32(const float *rois, const float *box_out, int ld, int loc0, const int32_t *prev_label, int N, int S,
                             const float *loc_mean4, const float *std_prev4 /* host */, const float *per_image_hw, float img_h, float img_w,
                             const float *gt_boxes, const int32_t *gt_labels, const int32_t *n_gt, int gt_cap, float iou_thresh,
                             const float *std_next4 /* host */, float *roi, float *rois_xy5, int32_t *levels, float *gt_loc, int32_t *label,
                             int32_t *gt_assign, void *stream);
int mrcnn_cascade_prob_f32(const float *box_out0, const float *box_out1, const float *box_out2, const float *box_out3, int K, int R, int ld,
                           int n_class, float *prob, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mask Scoring R-CNN (maskiou.hip; no counterpart in the reference).  Integer counts, float32 without contraction,
 * correctly rounded divisions, no float atomics: the same bits on every run.  Every launch is capture-safe.
 * n_channels: the logical class channels a label may select (label - label_base in [0, n_channels)); MRCNN_E_INVALID when it is not in
 *   [1, Cp] / [1, ld].  label_base: 1 for the sampler's labels (0 = background), 0 for the labels MaskRCNN.predict returns.  A row whose
 *   channel is outside [0, n_channels) has no class: target 0 with zero counts, logit channel 0, no loss and a zero gradient row.
 * maskiou_target: two launches.  masks (N,G,H,W) u8; n_gt (N) device; sample_roi (N*n_sample,4) (y1,x1,y2,x2), gt_assign (N*n_sample),
 *   n_pos (N): the sampler's outputs; the mask block has Rm = N * rows rows, row r being sampler row (r / rows) * n_sample + r % rows;
 *   label (Rm), mask_out (Rm,mask_size,mask_size,Cp), gt_roi_mask (Rm,mask_size,mask_size) int32.
 *   (a) area (N,G) int32 = nonzero bytes of every mask with g < n_gt[i], 0 for the other slots whatever they hold: 16-byte loads between
 *   a byte-wise head and tail, reduced in the wave, 32 partial counts per mask in ws (mrcnn_maskiou_target_workspace_bytes).
 *   (b) one workgroup per row; full = area of the assigned mask, crop = nonzero bytes of it inside the rectangle mrcnn_mask_target_u8
 *   crops (y0 = max((int)y1, 0), y1 = min((int)y2, H), x alike), pred = #(logit at the row's channel > 0), gt28 = #(gt_roi_mask > 0),
 *   ovr = #(both);  full_est = ((float)gt28 * (float)full) / (float)crop;  uni = ((float)pred + full_est) - (float)ovr;
 *   target = (float)ovr / fmaxf(uni, 1.0f).  target = 0 where crop == 0, full == 0, the rectangle is empty or the row is padding
 *   (r % rows >= n_pos[i], no channel, gt_assign outside [0, min(G, n_gt[i]))).  counts (Rm,5) int32, nullable: (full, crop, pred, gt28, ovr), zeros
 *   for padding rows.  rows == 0 succeeds without a launch.
 * maskiou_input_fwd: feat (Rm,P,P,C), mask_out (Rm,2P,2P,Cp) -> out (Rm,P,P,cin_p): channels [0,C) = feat, channel C =
 *   fmaxf(fmaxf(fmaxf(m[2y][2x], m[2y][2x+1]), m[2y+1][2x]), m[2y+1][2x+1]) of the row's channel (0 for a row without one), channels
 *   (C,cin_p) = 0.  C and cin_p multiples of 4, cin_p >= C + 4.
 * maskiou_input_bwd: g_pool (Rm,P,P,C) += g_in (Rm,P,P,cin_p)[..., :C], one float32 add per element.
 * maskiou_l2: over the rows with target > 0 and a channel, d = pred[r*ld + channel] - target[r]: loss_out[0] = weight * sum(0.5 d^2) / count,
 *   loss_out[1] = max(count, 1) (the (sum, count) form of mrcnn_smooth_l1_f32: block partials, one finalising wave in double);
 *   gx (Rm,ld), nullable: d * (weight * (1 / loss_out[1])) at that column, 0 in every other element.  No such row: loss 0, gx 0.
 *   ws: mrcnn_loss_workspace_bytes().
 * maskiou_rescore: out[d] = score[d] * fminf(fmaxf(pred[d*ld + label[d]], 0), 1); label 0-based; a label outside [0, n_channels) gives 0.
 * Rm == 0 / D == 0 succeed without a launch.
 * ---------------------------------------------------------------------------------------- */
size_t mrcnn_maskiou_target_workspace_bytes(int N, int G);
int mrcnn_maskiou_target(const uint8_t *masks, int N, int G, int H, int W, const int32_t *n_gt, const float *sample_roi,
                         const int32_t *gt_assign, const int32_t *label, const int32_t *n_pos, int n_sample, int rows,
                         const float *mask_out, int mask_size, int Cp, int n_channels, const int32_t *gt_roi_mask, int label_base,
                         int32_t *area, float *target, int32_t *counts, void *ws, size_t ws_bytes, void *stream);
int mrcnn_maskiou_input_fwd(const float *feat, const float *mask_out, const int32_t *label, int label_base, int Rm, int P, int C, int Cp,
                            int n_channels, int cin_p, float *out, void *stream);
int mrcnn_maskiou_input_bwd(const float *g_in, int Rm, int P, int C, int cin_p, float *g_pool, void *stream);
int mrcnn_maskiou_l2(const float *pred, int ld, int n_channels, const float *target, const int32_t *label, int label_base, int Rm,
                     float weight, float *loss_out, float *gx, void *ws, size_t ws_bytes, void *stream);
int mrcnn_maskiou_rescore(const float *score, const float *pred, int ld, int n_channels, const int32_t *label, int D, float *out,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * PointRend mask refinement (pointrend.hip, point_common.h; no counterpart in the reference).  float32 without
 * contraction, no float atomics: the same bits on every run.  Every launch is capture-safe.  Zero rows / detections succeed without a launch.
 * point_sample(map, px, py): pixel centres at i + 0.5; fx = px - 0.5, x0 = floor(fx), lx = fx - x0, the same in y; taps (y0,x0), (y0,x0+1),
 *   (y0+1,x0), (y0+1,x0+1) with weights (1-ly)(1-lx), (1-ly)lx, ly(1-lx), ly*lx; a tap outside the map is zero and is not read; the four
 *   products are added in that order.
 * A row's box is its rois_xy5 entry (idx, x1, y1, x2, y2); the normalised point (u, v) has frame position X = x1 + u * (x2 - x1),
 *   Y = y1 + v * (y2 - y1).  coords (rows, P, 2) = (u, v).  n_channels: the logical class channels (label - label_base in [0, n_channels));
 *   MRCNN_E_INVALID when it is not in [1, Cp] / [1, ld].
 * point_train_coords: keys (rows, n_keys) uint32, n_keys >= 2 * n_cand + 2 * (P - n_imp); a key gives (key >> 8) * 2^-24.  Candidate j
 *   = keys (2j, 2j+1); its uncertainty is -|point_sample(coarse[r, :, :, label[r] - label_base], u * S0, v * S0)|, 0 for a row without a
 *   channel.  Points [0, n_imp): the most uncertain candidates, the most uncertain first, ties to the lower index (a bitonic sort of
 *   (bits of |value|, j) in LDS; n_cand <= 4096).  Points [n_imp, P): the keys 2 * n_cand + 2 * (p - n_imp) and the next.
 * point_features_fwd: out (rows, P, cin_p): [0, C) = point_sample of map (N,H,W,C), image idx, at (X * scale, Y * scale) (zeros for an idx
 *   outside [0, N)); [C, C + n_channels) = point_sample of coarse (rows,S0,S0,Cp) at (u * S0, v * S0); zeros behind.  C, Cp, cin_p
 *   multiples of 4.
 * point_features_bwd: g_map (N,H,W,C) += the transpose of the fine sampling applied to g_in (rows, P, ld)[..., :C].  Owner-computes: a wave
 *   owns 2 x 4 cells, scans the rows whose box in map coordinates, widened by one cell, touches them and adds w * g per tap in ascending
 *   (row, point) order, taps in the order above; the value the map held is the FIRST addend; every touched cell is written once, an
 *   untouched patch is neither read nor written.  C <= 512.
 * point_concat_fwd: out (n, cin_p) = [h (n, Ch) | x0 (n, ld0)[c0 : c0 + n_coarse] | zeros];  point_concat_bwd: g_h (n, Ch) = g_in (n, cin_p)[:, :Ch].
 * point_target: target (N * rows, P) = point_sample at (X, Y) of masks (N,G,H,W) u8 [i, gt_assign[i * n_sample + j]] read as 1.0 / 0.0; -1
 *   for a row that is not live (mrcnn_maskiou_target's rule: j < n_pos[i], label > 0, assignment in [0, min(G, n_gt[i]))).
 * point_bce: over the points with target >= 0 of rows with a channel, x = pred[(r * P + p) * ld + channel]: loss_out[0] = weight * sum(BCE
 *   with logits(x, t)) / count, loss_out[1] = max(count, 1) (block partials + one finalising wave in double, as mrcnn_smooth_l1_f32); gx
 *   (rows * P, ld), nullable: (sigmoid(x) - t) * (weight * (1 / loss_out[1])) in that column, 0 in every other element.  ws:
 *   mrcnn_loss_workspace_bytes().
 * point_subdivide: one workgroup per detection, S <= 56.  up (D, 2S, 2S)[y][x] = the channel label[d] (0 for a null label array) of grid
 *   (D,S,S,ld) at the centre ((x + 0.5) / 2, (y + 0.5) / 2), the weights and order of point_sample with the tap indices CLAMPED to the grid.
 *   The n_sel <= 4 S^2 cells of smallest |up|, ties to the lower flat index, in ASCENDING flat index: index (D, n_sel) int32, coords
 *   (D, n_sel, 2) = ((x + 0.5) / 2S, (y + 0.5) / 2S).
 * point_scatter: grid (D, cells)[d, index[d, j]] = pred (D * n_sel, ld)[d * n_sel + j, label[d]].
 * ---------------------------------------------------------------------------------------- */
int mrcnn_point_train_coords(const uint32_t *keys, int n_keys, const float *coarse, int S0, int Cp, int n_channels, const int32_t *label,
                             int label_base, int rows, int P, int n_cand, int n_imp, float *coords, void *stream);
int mrcnn_point_features_fwd(const float *coords, const float *rois_xy5, const float *map, int N, int H, int W, int C, float scale,
                             const float *coarse, int S0, int Cp, int n_channels, int rows, int P, int cin_p, float *out, void *stream);
int mrcnn_point_features_bwd(const float *g_in, int ld, const float *coords, const float *rois_xy5, int rows, int P, float scale, float *g_map,
                             int N, int H, int W, int C, void *stream);
int mrcnn_point_concat_fwd(const float *h, int Ch, const float *x0, int ld0, int c0, int n_coarse, long long n_points, int cin_p, float *out,
                           void *stream);
int mrcnn_point_concat_bwd(const float *g_in, int cin_p, int Ch, long long n_points, float *g_h, void *stream);
int mrcnn_point_target(const uint8_t *masks, int N, int G, int H, int W, const int32_t *n_gt, const float *rois_xy5, const int32_t *gt_assign,
                       const int32_t *label, const int32_t *n_pos, int n_sample, int rows, const float *coords, int P, float *target,
                       void *stream);
int mrcnn_point_bce(const float *pred, int ld, int n_channels, const float *target, const int32_t *label, int label_base, int rows, int P,
                    float weight, float *loss_out, float *gx, void *ws, size_t ws_bytes, void *stream);
int mrcnn_point_subdivide(const float *grid, int D, int S, int ld, int n_channels, const int32_t *label, int n_sel, float *up, int32_t *index,
                          float *coords, void *stream);
int mrcnn_point_scatter(const float *pred, int ld, int n_channels, const int32_t *label, const int32_t *index, int D, int n_sel, int cells,
                        float *grid, void *stream);

/* ----------------------------------------------------------------------------------------
 * Deformable convolution (v1) and its modulated form (v2) around a 3x3, stride 1, pad 1, dilation 1 layer with one deformable group
 * (csrc/deform.hip, csrc/deform_common.h).  No counterpart in the reference.  Every other KH, KW, stride, pad,
 * dilation or groups: MRCNN_E_UNSUPPORTED.  The GEMM of the layer is the caller's: mrcnn_conv2d_* as a 1x1 layer over cols.
 * x (N,H,W,C) NHWC, C % 4 == 0.  off (N,H,W,ld_off): for output pixel (n, y, x) and tap k = 3 * i + j, channels 2k, 2k + 1 = (dy, dx) and,
 *   modulated, channel 18 + k = a logit; only these 18 / 27 channels are read (ld_off >= that).  The sampling position is
 *   (y - 1 + i + dy, x - 1 + j + dx); the sample is the bilinear interpolation of the four cells around it, a cell outside the map counting
 *   as zero, times sigmoid(logit) when modulated.  Positions are compared in float before any conversion to an integer: a position at or
 *   beyond -1 or H (W), a huge or a non-finite offset samples zero, has a zero gradient and never indexes memory.
 * deform_cols_fwd: cols (N,H,W,9*C), tap-major: cols[n, y, x, k * C + c] = the sample of channel c at tap k.  One launch.
 * deform_offset_bwd: g_off (N,H,W,ld_off), the WHOLE row: channels 2k, 2k + 1 = m * sum_c g_cols * d sample / d (py, px), modulated channel
 *   18 + k = m (1 - m) * sum_c g_cols * sample, every other channel 0.  A wave reduction over the channels in a fixed order.  One launch.
 * deform_input_bwd: gx (N,H,W,C) = [accumulate: the value gx held, first] + the sum over every (source pixel, tap, corner) that touches the
 *   cell, in ascending (source pixel, tap, corner) order, of weight * m * g_cols; relu_x (N,H,W,C), nullable: the TOTAL is zeroed where
 *   relu_x <= 0.  No float atomics - the same bits on every run: an inverted index is built per call in ws (counts by integer atomics, an
 *   exclusive scan, a fill), each destination's list is ordered and summed by one wave; a list of more than 256 entries is ordered and
 *   summed by one workgroup in chunks of 128 entries whose partial sums are added in chunk order.  C <= 512.  One memset, five launches.
 *   ws: mrcnn_deform_input_bwd_workspace_bytes(N, H, W) bytes (0 for sizes the call refuses), 16-byte aligned.
 * x, cols, g_cols, gx, relu_x 16-byte aligned.  N == 0 succeeds without a launch.  Errors, before any launch: MRCNN_E_UNSUPPORTED for the
 * geometry above, N * H * W * 36 above 2^31 - 1, H or W above 2^20, C > 512 (input_bwd); MRCNN_E_INVALID for a modulated / accumulate outside
 * 0..1, a negative N, a non-positive H, W, C, C % 4 != 0, ld_off below 18 / 27, a NULL or misaligned pointer; MRCNN_E_WORKSPACE for a short
 * or NULL workspace.
 * ---------------------------------------------------------------------------------------- */
int mrcnn_deform_cols_fwd_f32(const float *x, const float *off, int ld_off, int modulated, int N, int H, int W, int C, int KH, int KW, int stride,
                              int pad, int dilation, int groups, float *cols, void *stream);
int mrcnn_deform_offset_bwd_f32(const float *g_cols, const float *x, const float *off, int ld_off, int modulated, int N, int H, int W, int C,
                                int KH, int KW, int stride, int pad, int dilation, int groups, float *g_off, void *stream);
size_t mrcnn_deform_input_bwd_workspace_bytes(int N, int H, int W);
int mrcnn_deform_input_bwd_f32(const float *g_cols, const float *off, int ld_off, int modulated, int N, int H, int W, int C, int KH, int KW,
                               int stride, int pad, int dilation, int groups, float *gx, const float *relu_x, int accumulate, void *ws,
                               size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MRCNN_HIP_H */
