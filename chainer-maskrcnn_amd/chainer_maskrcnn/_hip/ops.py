"""1:1 torch-tensor wrappers over the C ABI (include/mrcnn_hip.h) for everything except the
convolutions (``nn.py``) and ROIAlign (``functions/roi_align``).  Tensors are device-memory handles
only: every function checks the device, allocates outputs with ``torch.empty`` and launches HIP
kernels on the current stream.  No arithmetic happens in torch.
"""
import ctypes

import numpy as np
import torch

from chainer_maskrcnn import _hip
from chainer_maskrcnn._hip import lib, check, ptr, stream_ptr
from chainer_maskrcnn._hip.nn import workspace

f32 = torch.float32
i32 = torch.int32


def _empty(shape, dev, dtype=f32):
    return torch.empty(shape, dtype=dtype, device=dev)


def _ck(*ts):
    _hip.require_cuda(*ts)
    for t in ts:
        if t is not None and not t.is_contiguous():
            raise ValueError('non-contiguous tensor passed to a HIP op')


# ---- batch norm ---------------------------------------------------------------------------------
def bn_train_fwd(x, gamma, beta, residual=None, relu=False, running_mean=None, running_var=None,
                 eps=2e-5, decay=0.9):
    """x (..., C) NHWC.  Returns (y, save_mean, save_invstd)."""
    _ck(x, gamma, beta, residual)
    C = x.shape[-1]
    P = x.numel() // C
    y = torch.empty_like(x)
    mean = _empty((C,), x.device)
    invstd = _empty((C,), x.device)
    nb = lib().mrcnn_bn_workspace_bytes(P, C)
    ws = workspace(nb, x.device)
    check(lib().mrcnn_bn_train_fwd_f32(ptr(x), ptr(gamma), ptr(beta), ptr(residual), ptr(y), ptr(mean), ptr(invstd),
                                       ptr(running_mean), ptr(running_var), P, C, eps, decay, int(relu), ptr(ws),
                                       ws.numel(), stream_ptr()))
    return y, mean, invstd


def bn_train_fwd_stats(x, part, gamma, beta, residual=None, relu=False, running_mean=None, running_var=None, eps=2e-5, decay=0.9):
    """bn_train_fwd from the partial statistics (rows, 2, C) the producing convolution's epilogue left (hnn.conv2d_fwd_bnstats_raw)."""
    _ck(x, part, gamma, beta, residual)
    C = x.shape[-1]
    P = x.numel() // C
    y = torch.empty_like(x)
    mean = _empty((C,), x.device)
    invstd = _empty((C,), x.device)
    check(lib().mrcnn_bn_train_fwd_stats_f32(ptr(x), ptr(part), part.shape[0], ptr(gamma), ptr(beta), ptr(residual), ptr(y), ptr(mean),
                                             ptr(invstd), ptr(running_mean), ptr(running_var), P, C, eps, decay, int(relu), stream_ptr()))
    return y, mean, invstd


def bn_train_bwd(gy, x, y, gamma, mean, invstd, relu=False, want_gres=False, beta=None, gg=None, gb=None):
    """y None + beta given (BN + ReLU without residual): the ReLU mask is recomputed from x.  gg / gb: where the gradients of gamma /
    beta are written (the flat gradient buffer's views); allocated when not given."""
    _ck(gy, x, y, gamma, mean, invstd, beta, gg, gb)
    C = x.shape[-1]
    P = x.numel() // C
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if want_gres else None
    gg = _empty((C,), x.device) if gg is None else gg
    gb = _empty((C,), x.device) if gb is None else gb
    ws = workspace(lib().mrcnn_bn_workspace_bytes(P, C), x.device)
    check(lib().mrcnn_bn_train_bwd_f32(ptr(gy), ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(gx), ptr(gres),
                                       ptr(gg), ptr(gb), P, C, int(relu), ptr(ws), ws.numel(), stream_ptr()))
    return gx, gres, gg, gb


def bn_infer_fwd(x, gamma, beta, mean, var, residual=None, relu=False, eps=2e-5):
    _ck(x, gamma, beta, mean, var, residual)
    C = x.shape[-1]
    y = torch.empty_like(x)
    check(lib().mrcnn_bn_infer_fwd_f32(ptr(x), ptr(gamma), ptr(beta), ptr(mean), ptr(var), ptr(residual), ptr(y),
                                       x.numel() // C, C, eps, int(relu), stream_ptr()))
    return y


def bn_frozen_bwd(gy, gamma, var, yx=None, beta=None, mean=None, relu=0, want_gres=False, out=None, eps=2e-5):
    """Backward of a frozen (inference-mode) BatchNorm: gx = dz * gamma / sqrt(var + eps); relu 0 / 1 (yx = y) / 2 (yx = x, needs beta
    and mean).  out may be gy.  Returns (gx, gres or None)."""
    _ck(gy, gamma, var, yx, beta, mean, out)
    C = gy.shape[-1]
    gx = torch.empty_like(gy) if out is None else out
    gres = torch.empty_like(gy) if want_gres else None
    check(lib().mrcnn_bn_frozen_bwd_f32(ptr(gy), ptr(yx), ptr(gamma), ptr(beta), ptr(mean), ptr(var), ptr(gx), ptr(gres),
                                        gy.numel() // C, C, eps, int(relu), stream_ptr()))
    return gx, gres


def bn_infer_fwd_pair(xa, gamma_a, beta_a, mean_a, var_a, xb, gamma_b, beta_b, mean_b, var_b, eps=2e-5):
    """relu(bn_a(xa) + bn_b(xb)) with running statistics: the bits of bn_infer_fwd(xb) then bn_infer_fwd(xa, residual, relu)."""
    _ck(xa, gamma_a, beta_a, mean_a, var_a, xb, gamma_b, beta_b, mean_b, var_b)
    if xa.shape != xb.shape:
        raise ValueError('bn_infer_fwd_pair: xa %r and xb %r differ in shape' % (tuple(xa.shape), tuple(xb.shape)))
    C = xa.shape[-1]
    y = torch.empty_like(xa)
    check(lib().mrcnn_bn_infer_fwd_pair_f32(ptr(xa), ptr(gamma_a), ptr(beta_a), ptr(mean_a), ptr(var_a), ptr(xb), ptr(gamma_b),
                                            ptr(beta_b), ptr(mean_b), ptr(var_b), ptr(y), xa.numel() // C, C, eps, stream_ptr()))
    return y


def bn_frozen_bwd_pair(gy, y, gamma_a, var_a, gamma_b, var_b, out_a=None, eps=2e-5):
    """Both input gradients of relu(bn_a(xa) + bn_b(xb)) (frozen layers) from one read of gy and of y (None: gy arrives masked).
    out_a may be gy."""
    _ck(gy, y, gamma_a, var_a, gamma_b, var_b, out_a)
    C = gy.shape[-1]
    gxa = torch.empty_like(gy) if out_a is None else out_a
    gxb = torch.empty_like(gy)
    check(lib().mrcnn_bn_frozen_bwd_pair_f32(ptr(gy), ptr(y), ptr(gamma_a), ptr(var_a), ptr(gamma_b), ptr(var_b), ptr(gxa), ptr(gxb),
                                             gy.numel() // C, C, eps, stream_ptr()))
    return gxa, gxb


# ---- group norm (RoI heads; csrc/groupnorm.hip) ---------------------------------------------------
GN_PATHS = ('register', 'generic')      # values of group_norm_plan's path


def group_norm_plan(R, H, W, C, Cp, G):
    """(path, backward workspace bytes) of mrcnn_group_norm_plan: host arithmetic, no device.  Raises on an invalid geometry."""
    path, nb = ctypes.c_int(-1), ctypes.c_size_t(0)
    check(lib().mrcnn_group_norm_plan(int(R), int(H), int(W), int(C), int(Cp), int(G), ctypes.byref(path), ctypes.byref(nb)))
    return path.value, nb.value


def group_norm_fwd(x, gamma, beta, C, G, relu=False, want_stats=True, eps=1e-5):
    """x (R,H,W,Cp) NHWC with C logical channels in G groups.  Returns (y, mean, rstd); mean / rstd (R,G) are None unless want_stats."""
    _ck(x, gamma, beta)
    R, H, W, Cp = x.shape
    y = torch.empty_like(x)
    mean = _empty((R, G), x.device) if want_stats else None
    rstd = _empty((R, G), x.device) if want_stats else None
    check(lib().mrcnn_group_norm_fwd_f32(ptr(x), ptr(gamma), ptr(beta), R, H, W, int(C), Cp, int(G), eps, int(bool(relu)), ptr(y),
                                         ptr(mean), ptr(rstd), stream_ptr()))
    return y, mean, rstd


def group_norm_bwd(gy, x, gamma, beta, mean, rstd, C, G, relu=False, gg=None, gb=None, accumulate_params=False):
    """relu: recompute the ReLU mask from x (False: gy arrives masked, or the layer has no ReLU).  gg / gb: where the gradients of gamma /
    beta are written, or added with accumulate_params (the flat gradient buffer's views); allocated when not given.  Returns (gx, gg, gb)."""
    _ck(gy, x, gamma, beta, mean, rstd, gg, gb)
    R, H, W, Cp = x.shape
    if tuple(gy.shape) != tuple(x.shape):
        raise ValueError('group_norm_bwd: gy %r and x %r differ in shape' % (tuple(gy.shape), tuple(x.shape)))
    if (gg is None or gb is None) and accumulate_params:
        raise ValueError('group_norm_bwd: accumulate_params needs gg and gb')
    gx = torch.empty_like(x)
    gg = _empty((Cp,), x.device) if gg is None else gg
    gb = _empty((Cp,), x.device) if gb is None else gb
    _, nb = group_norm_plan(R, H, W, C, Cp, G)
    if R == 0 and not accumulate_params:        # the library launches nothing for an empty batch: the sums over no sample are zeros
        gg.zero_()
        gb.zero_()
    ws = workspace(nb, x.device)
    check(lib().mrcnn_group_norm_bwd_f32(ptr(gy), ptr(x), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), R, H, W, int(C), Cp, int(G),
                                         int(bool(relu)), ptr(gx), ptr(gg), ptr(gb), int(bool(accumulate_params)), ptr(ws), ws.numel(),
                                         stream_ptr()))
    return gx, gg, gb


# ---- group norm of whole maps (FPN; csrc/groupnorm_map.hip) ----------------------------------------
def group_norm_map_plan(R, H, W, C, Cp, G):
    """(pixels_per_chunk, chunks, forward workspace bytes, backward workspace bytes) of mrcnn_group_norm_map_plan: host arithmetic, no
    device.  Raises on an invalid geometry, and on one the map path does not take (C / G not a multiple of 4 up to 256, Cp above 1024)."""
    ppc, chunks, nf, nb = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib().mrcnn_group_norm_map_plan(int(R), int(H), int(W), int(C), int(Cp), int(G), ctypes.byref(ppc), ctypes.byref(chunks),
                                          ctypes.byref(nf), ctypes.byref(nb)))
    return ppc.value, chunks.value, nf.value, nb.value


def group_norm_map_fwd(x, gamma, beta, C, G, want_stats=True, eps=1e-5):
    """x (R,H,W,Cp) NHWC with C logical channels in G groups.  Returns (y, mean, rstd); mean / rstd (R,G) are None unless want_stats."""
    _ck(x, gamma, beta)
    R, H, W, Cp = x.shape
    y = torch.empty_like(x)
    mean = _empty((R, G), x.device) if want_stats else None
    rstd = _empty((R, G), x.device) if want_stats else None
    nf = group_norm_map_plan(R, H, W, C, Cp, G)[2]
    ws = workspace(nf, x.device)
    check(lib().mrcnn_group_norm_map_fwd_f32(ptr(x), ptr(gamma), ptr(beta), R, H, W, int(C), Cp, int(G), eps, ptr(y), ptr(mean), ptr(rstd),
                                             ptr(ws), ws.numel(), stream_ptr()))
    return y, mean, rstd


def group_norm_map_bwd(gy, x, gamma, mean, rstd, C, G, gg=None, gb=None, accumulate_params=False):
    """gg / gb: where the gradients of gamma / beta are written, or added with accumulate_params (the flat gradient buffer's views);
    allocated when not given.  Returns (gx, gg, gb)."""
    _ck(gy, x, gamma, mean, rstd, gg, gb)
    R, H, W, Cp = x.shape
    if tuple(gy.shape) != tuple(x.shape):
        raise ValueError('group_norm_map_bwd: gy %r and x %r differ in shape' % (tuple(gy.shape), tuple(x.shape)))
    if (gg is None or gb is None) and accumulate_params:
        raise ValueError('group_norm_map_bwd: accumulate_params needs gg and gb')
    gx = torch.empty_like(x)
    gg = _empty((Cp,), x.device) if gg is None else gg
    gb = _empty((Cp,), x.device) if gb is None else gb
    nb = group_norm_map_plan(R, H, W, C, Cp, G)[3]
    if R == 0 and not accumulate_params:        # the library launches nothing for an empty batch: the sums over no sample are zeros
        gg.zero_()
        gb.zero_()
    ws = workspace(nb, x.device)
    check(lib().mrcnn_group_norm_map_bwd_f32(ptr(gy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), R, H, W, int(C), Cp, int(G), ptr(gx), ptr(gg),
                                             ptr(gb), int(bool(accumulate_params)), ptr(ws), ws.numel(), stream_ptr()))
    return gx, gg, gb


def relu_bwd(gy, y, out=None):
    _ck(gy, y)
    out = torch.empty_like(gy) if out is None else out
    check(lib().mrcnn_relu_bwd_f32(ptr(gy), ptr(y), ptr(out), gy.numel(), stream_ptr()))
    return out


def add(a, b, out=None):
    _ck(a, b)
    out = torch.empty_like(a) if out is None else out
    check(lib().mrcnn_add_f32(ptr(a), ptr(b), ptr(out), a.numel(), stream_ptr()))
    return out


def maxpool2x2_fwd(x):
    _ck(x)
    N, H, W, C = x.shape
    y = _empty((N, (H + 1) // 2, (W + 1) // 2, C), x.device)
    check(lib().mrcnn_maxpool2x2_fwd_f32(ptr(x), ptr(y), N, H, W, C, stream_ptr()))
    return y


def maxpool3x3s2_fwd(x):
    """F.max_pooling_2d(ksize=3, stride=2) with cover_all (C4Backbone pool1)."""
    _ck(x)
    N, H, W, C = x.shape
    y = _empty((N, (H - 2) // 2 + 1, (W - 2) // 2 + 1, C), x.device)
    check(lib().mrcnn_maxpool3x3s2_fwd_f32(ptr(x), ptr(y), N, H, W, C, stream_ptr()))
    return y


def global_avg_pool(x):
    """x (R,H,W,C) -> (R,C): mean over the spatial positions."""
    _ck(x)
    R, H, W, C = x.shape
    y = _empty((R, C), x.device)
    check(lib().mrcnn_global_avg_pool_fwd_f32(ptr(x), ptr(y), R, H * W, C, stream_ptr()))
    return y


def relu(x, out=None):
    _ck(x)
    out = torch.empty_like(x) if out is None else out
    check(lib().mrcnn_relu_fwd_f32(ptr(x), ptr(out), x.numel(), stream_ptr()))
    return out


def maxpool2x2_bwd(x, gy):
    _ck(x, gy)
    N, H, W, C = x.shape
    gx = torch.empty_like(x)
    check(lib().mrcnn_maxpool2x2_bwd_f32(ptr(x), ptr(gy), ptr(gx), N, H, W, C, stream_ptr()))
    return gx


def upsample2x_add_fwd(top, lat):
    _ck(top, lat)
    N, H, W, C = lat.shape
    out = torch.empty_like(lat)
    check(lib().mrcnn_upsample2x_add_fwd_f32(ptr(top), ptr(lat), ptr(out), N, H, W, top.shape[1], top.shape[2], C,
                                             stream_ptr()))
    return out


def upsample2x_bwd(gout, gtop=None, top_shape=None):
    """gtop given => accumulate into it; else allocate (top_shape) and overwrite."""
    _ck(gout, gtop)
    N, H, W, C = gout.shape
    acc = gtop is not None
    if gtop is None:
        gtop = _empty(top_shape, gout.device)
    check(lib().mrcnn_upsample2x_bwd_f32(ptr(gout), ptr(gtop), N, H, W, gtop.shape[1], gtop.shape[2], C, int(acc),
                                         stream_ptr()))
    return gtop


def subsample_bwd(gsub, x_shape, stride, gx=None, relu_x=None):
    """relu_x (x_shape, nullable): the scattered positions are zeroed where relu_x <= 0 (after the accumulation); positions off
    the lattice keep what gx held - pass a gx that is already masked."""
    _ck(gsub, gx, relu_x)
    N, H, W, C = x_shape
    acc = gx is not None
    if gx is None:
        gx = _empty(x_shape, gsub.device)
    check(lib().mrcnn_subsample_bwd_f32(ptr(gsub), ptr(gx), N, H, W, C, stride, int(acc), ptr(relu_x), stream_ptr()))
    return gx


def pixel_shuffle2x(t, bias=None, inverse=False):
    """forward: t (N,H,W,4*C) [+ bias (C)] -> (N,2H,2W,C); inverse: (N,2H,2W,C) -> (N,H,W,4*C)."""
    _ck(t, bias)
    if not inverse:
        N, H, W, C4 = t.shape
        C = C4 // 4
        out = _empty((N, 2 * H, 2 * W, C), t.device)
    else:
        N, H2, W2, C = t.shape
        H, W = H2 // 2, W2 // 2
        out = _empty((N, H, W, 4 * C), t.device)
    check(lib().mrcnn_pixel_shuffle2x_f32(ptr(t), ptr(bias), ptr(out), N, H, W, C, int(inverse), stream_ptr()))
    return out


def bilinear2x_fwd(x):
    _ck(x)
    N, H, W, C = x.shape
    y = _empty((N, 2 * H, 2 * W, C), x.device)
    check(lib().mrcnn_bilinear2x_fwd_f32(ptr(x), ptr(y), N, H, W, C, stream_ptr()))
    return y


def bilinear2x_bwd(gy):
    _ck(gy)
    N, OH, OW, C = gy.shape
    gx = _empty((N, OH // 2, OW // 2, C), gy.device)
    check(lib().mrcnn_bilinear2x_bwd_f32(ptr(gy), ptr(gx), N, OH // 2, OW // 2, C, stream_ptr()))
    return gx


def image_nchw3_to_nhwc4(x):
    _ck(x)
    N, C, H, W = x.shape
    if C != 3:
        raise ValueError('expected (N,3,H,W) images')
    y = _empty((N, H, W, 4), x.device)
    check(lib().mrcnn_image_nchw3_to_nhwc4_f32(ptr(x), ptr(y), N, H, W, stream_ptr()))
    return y


def image_resize_f32(img, oh, ow, div=1.0):
    """img (C,H,W) float32 -> (C,oh,ow): cv2.resize INTER_LINEAR float rule, then / div (MaskRCNN.prepare)."""
    _ck(img)
    C, H, W = img.shape
    out = _empty((C, oh, ow), img.device)
    check(lib().mrcnn_image_resize_f32(ptr(img), C, H, W, ptr(out), oh, ow, oh, ow, float(div), stream_ptr()))
    return out


# ---- batched training resizes with an optional horizontal flip (augment.hip) -------------------------------------------------------
# mrcnn_resize_desc_t of include/mrcnn_hip.h, one row per example of the batch
RESIZE_DESC = np.dtype([('src_offset', '<i8'), ('H', '<i4'), ('W', '<i4'), ('oh', '<i4'), ('ow', '<i4'), ('flip', '<i4'), ('count', '<i4')])
assert RESIZE_DESC.itemsize == 32


def resize_descs(rows):
    """[(src_offset, H, W, oh, ow, flip, count)] -> the host descriptor table the two batched kernels take."""
    return np.array([tuple(int(v) for v in r) for r in rows], RESIZE_DESC)


def image_resize_batch_u8(src, desc, dst_h, dst_w, div=255.0):
    """src: 1-D uint8 device tensor holding the batch's (H,W,3) images packed at desc['src_offset']; desc: resize_descs(...).  Returns
    the zero-padded (N,3,dst_h,dst_w) float32 batch: resize_linear of each image, mirrored where desc['flip'] is 1, / div.  One launch."""
    _ck(src)
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError('image_resize_batch_u8: src must be a 1-D uint8 tensor')
    desc = np.ascontiguousarray(desc, RESIZE_DESC)
    N = len(desc)
    out = _empty((N, 3, dst_h, dst_w), src.device)
    check(lib().mrcnn_image_resize_batch_u8_f32(ptr(src), src.numel(), desc.ctypes.data, N, ptr(out), dst_h, dst_w, float(div),
                                                stream_ptr()))
    return out


def mask_resize_batch_u8(src, desc, G, dst_h, dst_w):
    """src: 1-D uint8 device tensor holding each example's (count,H,W) masks packed at desc['src_offset']; desc: resize_descs(...).
    Returns the zero-padded (N,G,dst_h,dst_w) uint8 batch: resize_nearest of each mask, mirrored where desc['flip'] is 1; rows past an
    example's count are zero.  One launch."""
    _ck(src)
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError('mask_resize_batch_u8: src must be a 1-D uint8 tensor')
    desc = np.ascontiguousarray(desc, RESIZE_DESC)
    N = len(desc)
    out = torch.empty((N, G, dst_h, dst_w), dtype=torch.uint8, device=src.device)
    check(lib().mrcnn_mask_resize_batch_nearest_u8(ptr(src) if src.numel() else ptr(None), src.numel(), desc.ctypes.data, N, G, ptr(out),
                                                   dst_h, dst_w, stream_ptr()))
    return out


# ---- large-scale jitter: the same resizes through a crop window (augment.hip) ---------------------------------------
# mrcnn_crop_desc_t of include/mrcnn_hip.h
CROP_DESC = np.dtype(RESIZE_DESC.descr + [('y0', '<i4'), ('x0', '<i4'), ('ch', '<i4'), ('cw', '<i4')])
assert CROP_DESC.itemsize == 48


def crop_descs(rows):
    """[(src_offset, H, W, oh, ow, flip, count, y0, x0, ch, cw)] -> the host descriptor table the crop kernels take."""
    return np.array([tuple(int(v) for v in r) for r in rows], CROP_DESC)


def _crop_src(name, src):
    _ck(src)
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError('%s: src must be a 1-D uint8 tensor' % name)
    return ptr(src) if src.numel() else ptr(None)


def image_resize_crop_batch_u8(src, desc, dst_h, dst_w, div=255.0):
    """image_resize_batch_u8 through each example's crop window (desc: crop_descs(...)): the window of the virtual oh x ow resize at the
    top-left of the (N,3,dst_h,dst_w) canvas, zero elsewhere.  One launch."""
    sp = _crop_src('image_resize_crop_batch_u8', src)
    desc = np.ascontiguousarray(desc, CROP_DESC)
    out = _empty((len(desc), 3, dst_h, dst_w), src.device)
    check(lib().mrcnn_image_resize_crop_batch_u8_f32(sp, src.numel(), desc.ctypes.data, len(desc), ptr(out), dst_h, dst_w, float(div),
                                                     stream_ptr()))
    return out


def mask_crop_boxes_u8(src, desc, labels_in, G, dst_h, dst_w):
    """What the crop leaves of each instance, without writing a plane.  src: each example's (count,H,W) masks packed at
    desc['src_offset']; labels_in (N,Gin) int32.  Returns (bboxes (N,G,4) float32, labels (N,G) int32, gather (N,G) int32): per example
    the instances with a pixel inside the window first, in their order, with the tight box of their cropped mask; behind them zero
    boxes, label -1 and gather -1.  One fill and two launches, no host synchronisation."""
    sp = _crop_src('mask_crop_boxes_u8', src)
    _ck(labels_in)
    desc = np.ascontiguousarray(desc, CROP_DESC)
    N = len(desc)
    if labels_in.dtype != i32 or labels_in.dim() != 2 or labels_in.shape[0] != N or not labels_in.is_contiguous():
        raise ValueError('mask_crop_boxes_u8: labels_in must be a contiguous (N,Gin) int32 tensor')
    Gin = labels_in.shape[1]
    bboxes, labels, gather = _empty((N, G, 4), src.device), _empty((N, G), src.device, i32), _empty((N, G), src.device, i32)
    ws = _empty((N, Gin, 4), src.device, i32)
    check(lib().mrcnn_mask_crop_boxes_u8(sp, src.numel(), desc.ctypes.data, N, Gin, G, dst_h, dst_w, ptr(labels_in), ptr(bboxes),
                                         ptr(labels), ptr(gather), ptr(ws), stream_ptr()))
    return bboxes, labels, gather


def mask_resize_crop_batch_u8(src, desc, gather, dst_h, dst_w):
    """mask_resize_batch_u8 through each example's crop window, output plane j reading source instance gather[n, j] (mask_crop_boxes_u8's
    table; -1: a zero plane).  Returns the (N,G,dst_h,dst_w) uint8 batch.  One launch."""
    sp = _crop_src('mask_resize_crop_batch_u8', src)
    _ck(gather)
    desc = np.ascontiguousarray(desc, CROP_DESC)
    N = len(desc)
    if gather.dtype != i32 or gather.dim() != 2 or gather.shape[0] != N or not gather.is_contiguous():
        raise ValueError('mask_resize_crop_batch_u8: gather must be a contiguous (N,G) int32 tensor')
    G = gather.shape[1]
    out = torch.empty((N, G, dst_h, dst_w), dtype=torch.uint8, device=src.device)
    check(lib().mrcnn_mask_resize_crop_batch_nearest_u8(sp, src.numel(), desc.ctypes.data, N, G, ptr(gather), ptr(out), dst_h, dst_w,
                                                        stream_ptr()))
    return out


# ---- Simple Copy-Paste on a large-scale-jitter batch (copy_paste.hip) ----------------------------------------------
def copy_paste(imgs, masks, labels, gather, sel, receive, G_out):
    """dataset.augment.copy_paste_batch on the device.  imgs (N,3,H,W) float32, masks (N,G,H,W) uint8, labels (N,G) int32 and gather
    (N,G) int32 as the LSJ stage leaves them (gather: the original instance index of each row), sel (N,Gin) uint8 (original instance i
    of example n is offered), receive (N,) uint8 (example n takes the offer of its partner (n + 1) % N).  Returns new tensors
    (imgs, masks (N,G_out,H,W), bboxes (N,G_out,4) float32, labels (N,G_out) int32); the inputs are only read.  One fill and four
    launches on the current stream, no host synchronisation."""
    _ck(imgs, masks, labels, gather, sel, receive)
    if imgs.dtype != f32 or imgs.dim() != 4 or imgs.shape[1] != 3:
        raise ValueError('copy_paste: imgs must be a contiguous (N,3,H,W) float32 tensor')
    N, _, H, W = imgs.shape
    if masks.dtype != torch.uint8 or masks.dim() != 4 or masks.shape[0] != N or tuple(masks.shape[2:]) != (H, W):
        raise ValueError('copy_paste: masks must be a contiguous (N,G,H,W) uint8 tensor of the images\' size')
    G = masks.shape[1]
    for name, t in (('labels', labels), ('gather', gather)):
        if t.dtype != i32 or tuple(t.shape) != (N, G):
            raise ValueError('copy_paste: %s must be a contiguous (N,G) int32 tensor' % name)
    if sel.dtype != torch.uint8 or sel.dim() != 2 or sel.shape[0] != N:
        raise ValueError('copy_paste: sel must be a contiguous (N,Gin) uint8 tensor')
    if receive.dtype != torch.uint8 or tuple(receive.shape) != (N,):
        raise ValueError('copy_paste: receive must be a contiguous (N,) uint8 tensor')
    Gin, G_out, dev = sel.shape[1], int(G_out), imgs.device
    if not 1 <= G_out <= 65535:         # (before anything is allocated or launched; the entry point refuses it as well)
        raise ValueError('copy_paste: G_out = %d outside 1..65535' % G_out)
    out_imgs, alpha = _empty((N, 3, H, W), dev), _empty((N, H, W), dev, torch.uint8)
    check(lib().mrcnn_copy_paste_image_f32(ptr(imgs), ptr(masks), ptr(labels), ptr(gather), ptr(sel), ptr(receive), N, G, Gin, H, W,
                                           ptr(out_imgs), ptr(alpha), stream_ptr()))
    out_masks = _empty((N, G_out, H, W), dev, torch.uint8)
    bboxes, out_labels, source = _empty((N, G_out, 4), dev), _empty((N, G_out), dev, i32), _empty((N, G_out), dev, i32)
    ws = _empty((N, 2 * G, 4), dev, i32)
    check(lib().mrcnn_copy_paste_masks_u8(ptr(masks), ptr(alpha), ptr(labels), ptr(gather), ptr(sel), ptr(receive), N, G, Gin, G_out, H, W,
                                          ptr(out_masks), ptr(bboxes), ptr(out_labels), ptr(source), ptr(ws), stream_ptr()))
    return out_imgs, out_masks, bboxes, out_labels


def random_keys(shape, seed, device):
    """uint32 sampler keys stored in an int32 tensor."""
    out = _empty(shape, device, i32)
    check(lib().mrcnn_random_keys_u32(ptr(out), out.numel(), int(seed) & (2 ** 64 - 1), stream_ptr()))
    return out


def seed_state(seed, device):
    """Device-resident sampler seed (int64 tensor of one element)."""
    return torch.tensor([int(seed) & (2 ** 63 - 1)], dtype=torch.int64, device=device)


def random_keys_dev(shape, state):
    """uint32 keys from the device seed state; advances the state (graph-replay safe)."""
    out = _empty(shape, state.device, i32)
    check(lib().mrcnn_random_keys_dev_u32(ptr(out), out.numel(), ptr(state), stream_ptr()))
    return out


class KeyStream(object):
    """A sampler's keys: ``seed`` and the device-resident ``state`` every draw advances (created by the first draw, and anew when the
    device changes).  The trainer state saves the two (MomentumSGD.state_dict, 'samplers')."""

    def __init__(self, seed):
        self.seed, self.state = seed, None

    def set_seed(self, seed, device=None):
        self.seed = seed
        self.state = None if device is None else seed_state(seed, device)

    def draw(self, shape, device):
        if self.state is None or self.state.device != device:
            self.state = seed_state(self.seed, device)
        return random_keys_dev(shape, self.state)


def sgd_momentum_wd(p, g, v, lr, momentum=0.9, weight_decay=5e-4):
    _ck(p, g, v)
    check(lib().mrcnn_sgd_momentum_wd_f32(ptr(p), ptr(g), ptr(v), p.numel(), lr, momentum, weight_decay, stream_ptr()))


def sgd_momentum_wd_masked(p, g, v, offset, frozen_blocks, lr, momentum=0.9, weight_decay=5e-4):
    """sgd_momentum_wd over a section (p, g, v: views starting at element ``offset`` of the flat buffers) that skips the 64-float blocks
    whose bit is set in ``frozen_blocks`` (int32 words over the WHOLE flat buffer, ParamStore.frozen_block_mask)."""
    _ck(p, g, v, frozen_blocks)
    check(lib().mrcnn_sgd_momentum_wd_masked_f32(ptr(p), ptr(g), ptr(v), p.numel(), int(offset), ptr(frozen_blocks),
                                                 frozen_blocks.numel() * 32, lr, momentum, weight_decay, stream_ptr()))


# the optimizer's device-resident hyper block (include/mrcnn_hip.h: MRCNN_HYPER_*)
HYPER_FLOATS, HYPER_LR, HYPER_A, HYPER_THRESHOLD, HYPER_SCALE, HYPER_NORM, HYPER_RATE, HYPER_SKIPPED = 8, 0, 1, 2, 3, 4, 5, 6


def _mask_args(frozen_blocks):
    return ptr(frozen_blocks), 0 if frozen_blocks is None else frozen_blocks.numel() * 32


def grad_accumulate(acc, g, offset=0, frozen_blocks=None, first=False):
    """acc = g (first) or acc += g over a section (views starting at element ``offset`` of the flat buffers); frozen blocks untouched."""
    _ck(acc, g, frozen_blocks)
    if acc.numel() != g.numel():
        raise ValueError('grad_accumulate: acc and g differ in size')
    mp, nb = _mask_args(frozen_blocks)
    check(lib().mrcnn_grad_accumulate_f32(ptr(acc), ptr(g), g.numel(), int(offset), mp, nb, int(first), stream_ptr()))


def grad_norm_workspace(n, device):
    """A workspace of its own for grad_norm_hyper over n elements (the optimizer keeps one: its partial sums never share a buffer)."""
    return torch.empty(max(int(lib().mrcnn_grad_norm_workspace_bytes(int(n))), 8), dtype=torch.uint8, device=device)


def grad_norm_hyper(g, hyper, acc=None, offset=0, frozen_blocks=None, ws=None):
    """The clipped-gradient scale of the WHOLE buffer into the hyper block: norm = sqrt(sum (acc + g)^2) * a in double, rate, scale
    (include/mrcnn_hip.h).  Nothing comes back to the host.  ws: grad_norm_workspace (default: the stream's scratch buffer)."""
    _ck(g, hyper, acc, frozen_blocks, ws)
    if hyper.numel() < HYPER_FLOATS or (acc is not None and acc.numel() != g.numel()):
        raise ValueError('grad_norm_hyper: hyper block too small, or acc and g differ in size')
    if ws is None:
        ws = workspace(lib().mrcnn_grad_norm_workspace_bytes(g.numel()), g.device)
    mp, nb = _mask_args(frozen_blocks)
    check(lib().mrcnn_grad_norm_hyper_f32(ptr(acc), ptr(g), g.numel(), int(offset), mp, nb, ptr(hyper), ptr(ws), ws.numel() * ws.element_size(),
                                          stream_ptr()))


def sgd_momentum_wd_hyper(p, g, v, hyper, acc=None, offset=0, frozen_blocks=None, momentum=0.9, weight_decay=5e-4):
    """sgd_momentum_wd of gs = (acc + g) * scale with the learning rate and the scale read from the hyper block on the device."""
    _ck(p, g, v, hyper, acc, frozen_blocks)
    if hyper.numel() < HYPER_FLOATS or g.numel() != p.numel() or v.numel() != p.numel() or (acc is not None and acc.numel() != p.numel()):
        raise ValueError('sgd_momentum_wd_hyper: hyper block too small, or the sections differ in size')
    mp, nb = _mask_args(frozen_blocks)
    check(lib().mrcnn_sgd_momentum_wd_hyper_f32(ptr(p), ptr(acc), ptr(g), ptr(v), p.numel(), int(offset), mp, nb, ptr(hyper), momentum,
                                                weight_decay, stream_ptr()))


# ---- losses -------------------------------------------------------------------------------------
def _loss_ws(dev):
    return workspace(lib().mrcnn_loss_workspace_bytes(), dev)


def softmax_ce_fills_gradient(M, K, xmap, gmap=None, Kfill=0):
    """True when mrcnn_softmax_ce_f32 takes its channel-interleaved path for these element maps (rows = (group, channel) over an NHWC
    (G, K, C) tensor: the keypoint loss) - the callee then writes EVERY element of gx (zeros in the padded channels and the ignored
    rows), so the caller need not zero-fill it.  Asks the library's own dispatch predicate (mrcnn_softmax_ce_fills_gx)."""
    A, gs, rs, es = xmap
    _, ggs, grs, ges = gmap or xmap
    return bool(lib().mrcnn_softmax_ce_fills_gx(int(M), int(K), int(A), int(gs), int(rs), int(es), int(ggs), int(grs), int(ges), int(Kfill)))


def softmax_ce(x, t, M, K, xmap, gmap=None, Kfill=0, want_grad=True, gx=None, ignore_label=-1, out=None):
    """x: device tensor holding a logical (M,K) matrix; xmap = (A, gs, rs, es) element map
    (see include/mrcnn_hip.h).  Returns (loss_out (2,), gx)."""
    _ck(t)
    _hip.require_cuda(x)
    out = _empty((2,), x.device) if out is None else out
    gmap = gmap or xmap
    if want_grad and gx is None:
        gx = torch.empty_like(x)
    ws = _loss_ws(x.device)
    check(lib().mrcnn_softmax_ce_f32(ptr(x), xmap[0], xmap[1], xmap[2], xmap[3], ptr(t), M, K, ignore_label, ptr(out),
                                     ptr(gx) if want_grad else None, gmap[1], gmap[2], gmap[3], Kfill, ptr(ws),
                                     ws.numel(), stream_ptr()))
    return out, gx


def smooth_l1(x, ldx, t, label, M, sigma, want_grad=True, gfill=0, col0=0, gx=None, out=None):
    """x: (M, ldx) buffer; the 4 predictions of row r start at column col0.  gx (same buffer shape) receives
    columns [col0, col0+max(4,gfill))."""
    _ck(x, t, label, gx)
    out = _empty((2,), x.device) if out is None else out
    if want_grad and gx is None:
        gx = torch.empty_like(x)
    ws = _loss_ws(x.device)
    xp = ctypes.c_void_p(x.data_ptr() + 4 * col0)
    gp = ctypes.c_void_p(gx.data_ptr() + 4 * col0) if want_grad else None
    check(lib().mrcnn_smooth_l1_f32(xp, ldx, ptr(t), ptr(label), M, sigma, ptr(out), gp, ldx, gfill, ptr(ws),
                                    ws.numel(), stream_ptr()))
    return out, gx


def box_iou_loss(x, ldx, t, rois, label, M, kind, mean, std, weight=1.0, roi_period=None, want_grad=True, gfill=0, col0=0, gx=None,
                 out=None):
    """GIoU / DIoU / CIoU on the decoded box (mrcnn_box_iou_loss_f32), with the buffers of ``smooth_l1``: x is an (M, ldx) buffer whose
    4 predicted deltas of row r start at column col0, t (M,4) the encoded targets, rois (roi_period,4) the boxes both are relative to
    (row r: rois[r % roi_period]; roi_period None = rois.shape[0]), mean / std the 4 normalisation constants of the encoding.  kind: a
    key of _hip.BOX_LOSS_KINDS or its value.  gx (same buffer shape) receives columns [col0, col0+max(4,gfill))."""
    _ck(x, t, rois, label, gx)
    kind = _hip.BOX_LOSS_KINDS.get(kind, kind)
    if roi_period is None:
        roi_period = rois.shape[0]
    if M > 0 and rois.numel() < 4 * roi_period:
        raise ValueError('box_iou_loss: rois holds %d boxes, roi_period is %d' % (rois.numel() // 4, roi_period))
    out = _empty((2,), x.device) if out is None else out
    if want_grad and gx is None:
        gx = torch.empty_like(x)
    ws = _loss_ws(x.device)
    xp = ctypes.c_void_p(x.data_ptr() + 4 * col0)
    gp = ctypes.c_void_p(gx.data_ptr() + 4 * col0) if want_grad else None
    f4 = ctypes.c_float * 4
    check(lib().mrcnn_box_iou_loss_f32(xp, ldx, ptr(t), ptr(rois), int(roi_period), ptr(label), M, int(kind), f4(*[float(v) for v in mean]),
                                       f4(*[float(v) for v in std]), float(weight), ptr(out), gp, ldx, gfill, ptr(ws), ws.numel(),
                                       stream_ptr()))
    return out, gx


def mask_bce(x, gt, label, want_grad=True, out=None):
    """x (Rm,H,W,Cm) NHWC logits, gt (Rm,H,W) int32, label (Rm,) int32."""
    _ck(x, gt, label)
    Rm, H, W, Cm = x.shape
    out = _empty((2,), x.device) if out is None else out
    gx = torch.empty_like(x) if want_grad else None
    ws = _loss_ws(x.device)
    check(lib().mrcnn_mask_bce_f32(ptr(x), ptr(gt), ptr(label), Rm, H * W, Cm, ptr(out), ptr(gx), ptr(ws), ws.numel(),
                                   stream_ptr()))
    return out, gx


def loss_total(losses):
    """losses (n,2) device pairs -> (1,) total."""
    _ck(losses)
    out = _empty((1,), losses.device)
    check(lib().mrcnn_loss_total_f32(ptr(losses), losses.shape[0], ptr(out), stream_ptr()))
    return out


# ---- RPN proposal path --------------------------------------------------------------------------
def rpn_pack(head, A, locs, scores, a_off):
    _ck(head, locs, scores)
    N, H, W, Cp = head.shape
    check(lib().mrcnn_rpn_pack_f32(ptr(head), N, H * W, Cp, A, ptr(locs), ptr(scores), a_off, locs.shape[1],
                                   stream_ptr()))


def rpn_pack_levels(heads, A, locs, scores):
    """All levels' head outputs (NHWC, same N and padded channel count) into locs / scores in ONE launch; level order = anchor order."""
    import ctypes
    _ck(locs, scores, *heads)
    L = len(heads)
    N, _, _, Cp = heads[0].shape
    ptrs = (ctypes.c_void_p * L)(*[h.data_ptr() for h in heads])
    hws = (ctypes.c_int * L)(*[h.shape[1] * h.shape[2] for h in heads])
    check(lib().mrcnn_rpn_pack_levels_f32(ptrs, hws, L, N, Cp, A, ptr(locs), ptr(scores), locs.shape[1], stream_ptr()))


def rpn_unpack_grad_levels(glocs, gscores, head_shapes, A):
    """The backward of rpn_pack_levels: one gradient tensor per level, one launch."""
    import ctypes
    _ck(glocs, gscores)
    L = len(head_shapes)
    N, _, _, Cp = head_shapes[0]
    gheads = [_empty(sh, glocs.device) for sh in head_shapes]
    ptrs = (ctypes.c_void_p * L)(*[g.data_ptr() for g in gheads])
    hws = (ctypes.c_int * L)(*[sh[1] * sh[2] for sh in head_shapes])
    check(lib().mrcnn_rpn_unpack_grad_levels_f32(ptr(glocs), ptr(gscores), ptrs, hws, L, N, Cp, A, glocs.shape[1], stream_ptr()))
    return gheads


def rpn_unpack_grad(glocs, gscores, head_shape, A, a_off):
    _ck(glocs, gscores)
    N, H, W, Cp = head_shape
    ghead = _empty(head_shape, glocs.device)
    check(lib().mrcnn_rpn_unpack_grad_f32(ptr(glocs), ptr(gscores), N, H * W, Cp, A, ptr(ghead), a_off, glocs.shape[1],
                                          stream_ptr()))
    return ghead


def rpn_proposals(locs, scores, anchors, img_size, min_size, n_pre, n_post, nms_thresh, debug=False, per_image=None):
    """locs (N,A,4), scores (N,A,2), anchors (A,4).  Returns dict of padded device outputs.
    per_image: optional (N,3) f32 device tensor (h, w, min_size * scale) - every image clipped / filtered with its own."""
    _ck(locs, scores, anchors, per_image)
    N, A, _ = locs.shape
    dev = locs.device
    rois = _empty((N * n_post, 4), dev)
    idx = _empty((N * n_post,), dev, i32)
    lev = _empty((N * n_post,), dev)
    cnt = _empty((N,), dev, i32)
    npre = min(n_pre, A)
    dbg = [None, None, None]
    if debug:
        dbg = [torch.full((N * npre,), -1, dtype=i32, device=dev), _empty((N * n_post,), dev, i32), _empty((N,), dev, i32)]
    ws = workspace(lib().mrcnn_rpn_proposals_workspace_bytes(N, A, n_pre, n_post), dev)
    check(lib().mrcnn_rpn_proposals_f32(ptr(locs), ptr(scores), ptr(anchors), N, A, float(img_size[0]),
                                        float(img_size[1]), float(min_size), ptr(per_image), n_pre, n_post, float(nms_thresh), ptr(rois),
                                        ptr(idx), ptr(lev), ptr(cnt), ptr(dbg[0]), ptr(dbg[1]), ptr(dbg[2]), ptr(ws),
                                        ws.numel(), stream_ptr()))
    return dict(rois=rois, roi_indices=idx, levels=lev, n_rois=cnt, sorted_anchor=dbg[0], keep=dbg[1], n_pre=dbg[2])


def softmax2(scores):
    """(..., 2) class scores -> softmax probabilities (the fg score of ChainerCV's single-level RPN)."""
    _ck(scores)
    out = torch.empty_like(scores)
    check(lib().mrcnn_softmax2_f32(ptr(scores), ptr(out), scores.numel() // 2, stream_ptr()))
    return out


def nms(boxes, thresh, max_keep=None):
    """Greedy NMS in the given order; returns (keep (max_keep,) int32 padded, n_keep (1,) int32)."""
    _ck(boxes)
    n = boxes.shape[0]
    max_keep = max_keep or max(n, 1)
    keep = torch.full((max_keep,), -1, dtype=i32, device=boxes.device)
    nk = _empty((1,), boxes.device, i32)
    ws = workspace(lib().mrcnn_nms_workspace_bytes(n), boxes.device)
    check(lib().mrcnn_nms_f32(ptr(boxes), n, float(thresh), max_keep, ptr(keep), ptr(nk), ptr(ws), ws.numel(),
                              stream_ptr()))
    return keep, nk


def map_rois_to_fpn_levels(rois, k_min=0, k_max=4):
    _ck(rois)
    lev = _empty((rois.shape[0],), rois.device)
    check(lib().mrcnn_map_rois_to_fpn_levels_f32(ptr(rois), rois.shape[0], k_min, k_max, ptr(lev), stream_ptr()))
    return lev


# ---- targets ------------------------------------------------------------------------------------
def proposal_target(rois, roi_levels, n_rois, gt_boxes, gt_labels, n_gt, keys, n_sample=256, pos_ratio=0.25,
                    pos_iou_thresh=0.5, neg_hi=0.5, neg_lo=0.0, mean=(0., 0., 0., 0.), std=(0.1, 0.1, 0.2, 0.2),
                    pos_order=None, neg_order=None):
    """rois (N*roi_cap,4) padded, gt_boxes (N,gt_cap,4), gt_labels (N,gt_cap) i32, keys (N,roi_cap+gt_cap) u32 (as int32
    storage).  Returns dict of per-row outputs (N*n_sample rows) + 'n_cand' (N,2) candidate-set sizes.
    pos_order / neg_order (N,n_sample) int32: reference-order mode (see include/mrcnn_hip.h), keys may be None."""
    _ck(rois, roi_levels, n_rois, gt_boxes, gt_labels, n_gt, keys, pos_order, neg_order)
    N, gt_cap = gt_labels.shape
    roi_cap = rois.shape[0] // N
    dev = rois.device
    R = N * n_sample
    o = dict(sample_roi=_empty((R, 4), dev), rois_xy5=_empty((R, 5), dev), sample_levels=_empty((R,), dev, i32),
             gt_roi_loc=_empty((R, 4), dev), gt_roi_label=_empty((R,), dev, i32), gt_assign=_empty((R,), dev, i32),
             sample_src=_empty((R,), dev, i32), n_pos=_empty((N,), dev, i32), n_sampled=_empty((N,), dev, i32),
             n_cand=_empty((N, 2), dev, i32))
    m4 = (ctypes.c_float * 4)(*mean)
    s4 = (ctypes.c_float * 4)(*std)
    import numpy as np
    n_pos_max = int(np.round(n_sample * pos_ratio))
    check(lib().mrcnn_proposal_target_f32(ptr(rois), ptr(roi_levels), ptr(n_rois), roi_cap, ptr(gt_boxes), ptr(gt_labels),
                                          ptr(n_gt), gt_cap, ptr(keys), N, n_sample, n_pos_max, pos_iou_thresh, neg_hi,
                                          neg_lo, ctypes.cast(m4, ctypes.c_void_p), ctypes.cast(s4, ctypes.c_void_p),
                                          ptr(o['sample_roi']), ptr(o['rois_xy5']), ptr(o['sample_levels']),
                                          ptr(o['gt_roi_loc']), ptr(o['gt_roi_label']), ptr(o['gt_assign']),
                                          ptr(o['sample_src']), ptr(o['n_pos']), ptr(o['n_sampled']), ptr(pos_order),
                                          ptr(neg_order), ptr(o['n_cand']), stream_ptr()))
    return o


def mask_target(masks, sample_roi, gt_assign, n_pos, n_sample, pos_cap, mask_size):
    """masks (N,gt_cap,H,W) uint8 -> (N*pos_cap, mask_size, mask_size) int32 (-1 rows for unused slots)."""
    _ck(masks, sample_roi, gt_assign, n_pos)
    N, gt_cap, H, W = masks.shape
    out = _empty((N * pos_cap, mask_size, mask_size), masks.device, i32)
    check(lib().mrcnn_mask_target_u8(ptr(masks), N, gt_cap, H, W, ptr(sample_roi), ptr(gt_assign), ptr(n_pos), n_sample,
                                     pos_cap, mask_size, ptr(out), stream_ptr()))
    return out


def keypoint_target(kps, sample_roi, gt_assign, n_pos, n_sample, pos_cap, mask_size, inplace_quirk=False):
    """kps (N,gt_cap,K,3) f32 -> (N*pos_cap, K) int32.  inplace_quirk: the reference's in-place gt mutation (App. B-11)."""
    _ck(kps, sample_roi, gt_assign, n_pos)
    N, gt_cap, K, _ = kps.shape
    out = _empty((N * pos_cap, K), kps.device, i32)
    check(lib().mrcnn_keypoint_target_f32(ptr(kps), N, gt_cap, K, ptr(sample_roi), ptr(gt_assign), ptr(n_pos), n_sample,
                                          pos_cap, mask_size, int(inplace_quirk), ptr(out), stream_ptr()))
    return out


def count_valid_labels(labels):
    """labels (N,G) int32 (-1 = padding row) -> per-image gt counts (N,) int32, on the device."""
    _ck(labels)
    N, G = labels.shape
    out = _empty((N,), labels.device, i32)
    check(lib().mrcnn_count_valid_labels_i32(ptr(labels), N, G, ptr(out), stream_ptr()))
    return out


def anchor_target(anchors, gt_boxes, n_gt, img_size, keys=None, n_sample=256, pos_iou_thresh=0.7, neg_iou_thresh=0.3,
                  pos_ratio=0.5, per_image_hw=None):
    """anchors (A,4), gt_boxes (N,gt_cap,4), keys (N,A) u32 or None (= no subsampling).  Returns (loc (N,A,4), label (N,A)).
    per_image_hw: optional (N,2) f32 device tensor - each image's own size for the inside test."""
    _ck(anchors, gt_boxes, n_gt, keys, per_image_hw)
    A = anchors.shape[0]
    N, gt_cap, _ = gt_boxes.shape
    dev = anchors.device
    loc = _empty((N, A, 4), dev)
    label = _empty((N, A), dev, i32)
    ws = workspace(lib().mrcnn_anchor_target_workspace_bytes(N, A), dev)
    check(lib().mrcnn_anchor_target_f32(ptr(anchors), A, ptr(gt_boxes), ptr(n_gt), gt_cap, N, float(img_size[0]),
                                        float(img_size[1]), ptr(per_image_hw), ptr(keys), n_sample, pos_iou_thresh, neg_iou_thresh, pos_ratio,
                                        int(keys is not None), ptr(loc), ptr(label), ptr(ws), ws.numel(), stream_ptr()))
    return loc, label


# ---- inference post-processing --------------------------------------------------------------------
def detect_decode(rois, box_out, n_class, loc0, scale, mean, std, size):
    """rois (R,4), box_out (R,ld) -> cls_bbox (R,4) in original-image pixels, prob (R,n_class)."""
    _ck(rois, box_out)
    R, ld = box_out.shape
    cls_bbox = _empty((R, 4), rois.device)
    prob = _empty((R, n_class), rois.device)
    m4 = (ctypes.c_float * 4)(*mean)
    s4 = (ctypes.c_float * 4)(*std)
    check(lib().mrcnn_detect_decode_f32(ptr(rois), R, ptr(box_out), ld, n_class, loc0, float(scale),
                                        ctypes.cast(m4, ctypes.c_void_p), ctypes.cast(s4, ctypes.c_void_p), float(size[0]),
                                        float(size[1]), ptr(cls_bbox), ptr(prob), stream_ptr()))
    return cls_bbox, prob


def cascade_refine(rois, box_out, loc0, N, mean, std_prev, size, prev_label=None, gt_boxes=None, gt_labels=None, n_gt=None,
                   iou_thresh=0.5, std_next=None):
    """One Cascade R-CNN stage to the next (mrcnn_cascade_refine_f32): rois (N*S,4) yx and the stage's box_out
    (N*S,ld) -> dict(roi (R,4), rois_xy5 (R,5), levels (R,) int32), and with gt_boxes (N,G,4) / gt_labels (N,G) i32 / n_gt (N,) i32 also
    gt_loc (R,4), label (R,) int32, gt_assign (R,) int32 at ``iou_thresh`` with ``std_next``.  size: an (N,2) float32 device tensor of
    each image's (h, w), or one (h, w) pair.  prev_label (R,) int32: rows with a label < 0 pass through as padding.  One launch."""
    hw = size if torch.is_tensor(size) else None
    _ck(rois, box_out, prev_label, gt_boxes, gt_labels, n_gt, hw)
    R, ld = box_out.shape
    N = int(N)
    if N < 0 or (N == 0 and R) or (N and R % N) or rois.numel() != R * 4:
        raise ValueError('cascade_refine: %d rows of box_out, %d boxes, %d images' % (R, rois.numel() // 4, N))
    S = R // N if N else 0
    train = gt_boxes is not None
    if train != (gt_labels is not None) or train != (n_gt is not None) or train != (std_next is not None):
        raise ValueError('cascade_refine: gt_boxes, gt_labels, n_gt and std_next go together')
    if train and (gt_boxes.dim() != 3 or gt_boxes.shape[0] != N or tuple(gt_labels.shape) != tuple(gt_boxes.shape[:2]) or n_gt.numel() != N):
        raise ValueError('cascade_refine: gt_boxes (N,G,4), gt_labels (N,G), n_gt (N,) expected for N = %d' % N)
    if prev_label is not None and prev_label.numel() != R:
        raise ValueError('cascade_refine: %d previous labels for %d rows' % (prev_label.numel(), R))
    if hw is not None and (hw.dtype != f32 or hw.numel() != 2 * N):
        raise ValueError('cascade_refine: per-image sizes are an (N,2) float32 tensor')
    dev = box_out.device
    o = dict(roi=_empty((R, 4), dev), rois_xy5=_empty((R, 5), dev), levels=_empty((R,), dev, i32))
    if train:
        o.update(gt_loc=_empty((R, 4), dev), label=_empty((R,), dev, i32), gt_assign=_empty((R,), dev, i32))
    m4 = (ctypes.c_float * 4)(*mean)
    sp4 = (ctypes.c_float * 4)(*std_prev)
    sn4 = (ctypes.c_float * 4)(*std_next) if train else None
    h, w = (0.0, 0.0) if hw is not None else (float(size[0]), float(size[1]))
    check(lib().mrcnn_cascade_refine_f32(ptr(rois), ptr(box_out), ld, int(loc0), ptr(prev_label), N, S, ctypes.cast(m4, ctypes.c_void_p),
                                         ctypes.cast(sp4, ctypes.c_void_p), ptr(hw), h, w, ptr(gt_boxes), ptr(gt_labels), ptr(n_gt),
                                         gt_boxes.shape[1] if train else 0, float(iou_thresh),
                                         ctypes.cast(sn4, ctypes.c_void_p) if train else ctypes.c_void_p(0), ptr(o['roi']),
                                         ptr(o['rois_xy5']), ptr(o['levels']), ptr(o.get('gt_loc')), ptr(o.get('label')),
                                         ptr(o.get('gt_assign')), stream_ptr()))
    return o


def cascade_prob(box_outs, n_class):
    """The inference score of a cascade (mrcnn_cascade_prob_f32): the K stages' box_out (R,ld) -> prob (R,n_class), the stages' softmax
    added in stage order and divided by K.  One launch."""
    _ck(*box_outs)
    K = len(box_outs)
    if not 2 <= K <= 4:
        raise ValueError('cascade_prob: %d stages (2 to 4)' % K)
    R, ld = box_outs[0].shape
    if any(tuple(b.shape) != (R, ld) for b in box_outs):
        raise ValueError('cascade_prob: the stages\' outputs differ in shape')
    prob = _empty((R, n_class), box_outs[0].device)
    p = [ptr(b) for b in box_outs] + [ctypes.c_void_p(0)] * (4 - K)
    check(lib().mrcnn_cascade_prob_f32(p[0], p[1], p[2], p[3], K, R, ld, int(n_class), ptr(prob), stream_ptr()))
    return prob


# ---- Mask Scoring R-CNN (maskiou.hip) -------------------------------------------------------------------------
def maskiou_target(masks, n_gt, sample_roi, gt_assign, label, n_pos, n_sample, rows, mask_out, gt_roi_mask, n_channels, label_base=1,
                   want_counts=False):
    """The MaskIoU regression target of every mask row (mrcnn_maskiou_target, two launches): masks (N,G,H,W) u8, n_gt (N,) i32, the
    sampler's sample_roi (N*n_sample,4) / gt_assign (N*n_sample,) / n_pos (N,), and the mask block's label (N*rows,), mask_out
    (N*rows,S,S,Cp) logits and gt_roi_mask (N*rows,S,S) i32 -> dict(target (Rm,) f32, area (N,G) i32[, counts (Rm,5) i32 = full, crop, pred,
    gt28, ovr])."""
    _ck(masks, n_gt, sample_roi, gt_assign, label, n_pos, mask_out, gt_roi_mask)
    if masks.dim() != 4 or masks.dtype != torch.uint8:
        raise ValueError('maskiou_target: masks are an (N,G,H,W) uint8 tensor')
    N, G, H, W = masks.shape
    rows, n_sample = int(rows), int(n_sample)
    Rm = N * rows
    if mask_out.dim() != 4 or mask_out.shape[0] != Rm or mask_out.shape[1] != mask_out.shape[2]:
        raise ValueError('maskiou_target: mask_out %r for %d rows' % (tuple(mask_out.shape), Rm))
    S, Cp = mask_out.shape[1], mask_out.shape[3]
    if label.numel() != Rm or gt_roi_mask.numel() != Rm * S * S or sample_roi.numel() != N * n_sample * 4 or gt_assign.numel() != N * n_sample \
            or n_pos.numel() != N or n_gt.numel() != N:
        raise ValueError('maskiou_target: the row counts of label / gt_roi_mask / sample_roi / gt_assign / n_pos / n_gt do not fit N = %d, '
                         'n_sample = %d, rows = %d' % (N, n_sample, rows))
    for t_, ty in ((n_gt, i32), (gt_assign, i32), (label, i32), (n_pos, i32), (gt_roi_mask, i32), (sample_roi, f32), (mask_out, f32)):
        if t_.dtype != ty:
            raise ValueError('maskiou_target: a %s tensor where %s is expected' % (t_.dtype, ty))
    dev = masks.device
    o = dict(target=_empty((Rm,), dev), area=_empty((N, G), dev, i32))
    if want_counts:
        o['counts'] = _empty((Rm, 5), dev, i32)
    nb = lib().mrcnn_maskiou_target_workspace_bytes(N, G)
    ws = workspace(nb, dev) if nb else None
    check(lib().mrcnn_maskiou_target(ptr(masks), N, G, H, W, ptr(n_gt), ptr(sample_roi), ptr(gt_assign), ptr(label), ptr(n_pos), n_sample,
                                     rows, ptr(mask_out), S, Cp, int(n_channels), ptr(gt_roi_mask), int(label_base), ptr(o['area']),
                                     ptr(o['target']), ptr(o.get('counts')), ptr(ws), ws.numel() if ws is not None else 0, stream_ptr()))
    return o


def maskiou_input_fwd(feat, mask_out, label, n_channels, cin_p, label_base=1):
    """The MaskIoU head's input (mrcnn_maskiou_input_fwd): feat (Rm,P,P,C) pooled features and mask_out (Rm,2P,2P,Cp) logits ->
    (Rm,P,P,cin_p): the features, the 2x2/2 max of the row's class logit in channel C, zeros behind it."""
    _ck(feat, mask_out, label)
    Rm, P, P2, C = feat.shape
    if P != P2 or tuple(mask_out.shape[:3]) != (Rm, 2 * P, 2 * P) or label.numel() != Rm or label.dtype != i32:
        raise ValueError('maskiou_input_fwd: feat %r, mask_out %r, %d labels' % (tuple(feat.shape), tuple(mask_out.shape), label.numel()))
    out = _empty((Rm, P, P, int(cin_p)), feat.device)
    check(lib().mrcnn_maskiou_input_fwd(ptr(feat), ptr(mask_out), ptr(label), int(label_base), Rm, P, C, mask_out.shape[3], int(n_channels),
                                        int(cin_p), ptr(out), stream_ptr()))
    return out


def maskiou_input_bwd(g_in, g_pool):
    """g_pool (Rm,P,P,C) += g_in (Rm,P,P,cin_p)[..., :C] in place (mrcnn_maskiou_input_bwd); returns g_pool."""
    _ck(g_in, g_pool)
    Rm, P, _, C = g_pool.shape
    if g_in.dim() != 4 or tuple(g_in.shape[:3]) != tuple(g_pool.shape[:3]):
        raise ValueError('maskiou_input_bwd: g_in %r against g_pool %r' % (tuple(g_in.shape), tuple(g_pool.shape)))
    check(lib().mrcnn_maskiou_input_bwd(ptr(g_in), Rm, P, C, g_in.shape[3], ptr(g_pool), stream_ptr()))
    return g_pool


def maskiou_l2(pred, target, label, n_channels, weight=1.0, label_base=1, want_grad=True, gx=None, out=None):
    """The MaskIoU loss (mrcnn_maskiou_l2): pred (Rm,ld), target (Rm,), label (Rm,) i32 -> (out (2,) = (weight * mean of 0.5 (x - t)^2 over
    the rows with target > 0, their count), gx (Rm,ld) with the gradient in the label's column and zeros elsewhere)."""
    _ck(pred, target, label, gx)
    Rm, ld = pred.shape
    if target.numel() != Rm or label.numel() != Rm or label.dtype != i32:
        raise ValueError('maskiou_l2: %d targets, %d labels for %d rows' % (target.numel(), label.numel(), Rm))
    out = _empty((2,), pred.device) if out is None else out
    if want_grad and gx is None:
        gx = torch.empty_like(pred)
    ws = _loss_ws(pred.device)
    check(lib().mrcnn_maskiou_l2(ptr(pred), ld, int(n_channels), ptr(target), ptr(label), int(label_base), Rm, float(weight), ptr(out),
                                 ptr(gx) if want_grad else None, ptr(ws), ws.numel(), stream_ptr()))
    return out, gx


def maskiou_rescore(score, pred, label, n_channels):
    """score (D,) * clamp(pred (D,ld)[d, label[d]], 0, 1) -> (D,) (mrcnn_maskiou_rescore); label (D,) i32, 0-based."""
    _ck(score, pred, label)
    D, ld = pred.shape
    if score.numel() != D or label.numel() != D or label.dtype != i32 or score.dtype != f32:
        raise ValueError('maskiou_rescore: %d scores, %d labels for %d rows' % (score.numel(), label.numel(), D))
    out = _empty((D,), pred.device)
    check(lib().mrcnn_maskiou_rescore(ptr(score), ptr(pred), ld, int(n_channels), ptr(label), D, ptr(out), stream_ptr()))
    return out


# ---- PointRend (pointrend.hip) --------------------------------------------------------------------------------
def point_n_keys(P, n_cand, n_imp):
    """uint32 keys per row mrcnn_point_train_coords reads: two per candidate and two per uniform point."""
    return 2 * int(n_cand) + 2 * (int(P) - int(n_imp))


def _point_dtypes(name, *pairs):
    for t_, ty in pairs:
        if t_ is not None and t_.dtype != ty:
            raise ValueError('%s: a %s tensor where %s is expected' % (name, t_.dtype, ty))


def point_train_coords(keys, coarse, label, n_channels, P, n_cand, n_imp, label_base=1):
    """The training points of every mask row (mrcnn_point_train_coords): keys (rows, point_n_keys) int32 holding uint32 bits, coarse
    (rows,S0,S0,Cp) logits, label (rows,) i32 -> coords (rows,P,2) (u, v) in [0,1): the n_imp most uncertain of n_cand candidates, the most
    uncertain first, then P - n_imp uniform points."""
    _ck(keys, coarse, label)
    rows = coarse.shape[0]
    if coarse.dim() != 4 or coarse.shape[1] != coarse.shape[2] or keys.dim() != 2 or keys.shape[0] != rows or label.numel() != rows:
        raise ValueError('point_train_coords: keys %r, coarse %r, %d labels' % (tuple(keys.shape), tuple(coarse.shape), label.numel()))
    _point_dtypes('point_train_coords', (keys, i32), (coarse, f32), (label, i32))
    coords = _empty((rows, int(P), 2), coarse.device)
    check(lib().mrcnn_point_train_coords(ptr(keys), keys.shape[1], ptr(coarse), coarse.shape[1], coarse.shape[3], int(n_channels), ptr(label),
                                         int(label_base), rows, int(P), int(n_cand), int(n_imp), ptr(coords), stream_ptr()))
    return coords


def point_features_fwd(coords, rois_xy5, fmap, scale, coarse, n_channels, cin_p):
    """The point head's input (mrcnn_point_features_fwd): coords (rows,P,2), rois_xy5 (rows,5), fmap (N,H,W,C) the stride-4 level, coarse
    (rows,S0,S0,Cp) -> (rows,1,P,cin_p): C fine channels, n_channels coarse channels, zeros."""
    _ck(coords, rois_xy5, fmap, coarse)
    rows, P = coords.shape[0], coords.shape[1]
    if coords.dim() != 3 or coords.shape[2] != 2 or tuple(rois_xy5.shape) != (rows, 5) or fmap.dim() != 4 or coarse.dim() != 4 \
            or coarse.shape[0] != rows or coarse.shape[1] != coarse.shape[2]:
        raise ValueError('point_features_fwd: coords %r, rois_xy5 %r, map %r, coarse %r' % (tuple(coords.shape), tuple(rois_xy5.shape),
                                                                                           tuple(fmap.shape), tuple(coarse.shape)))
    _point_dtypes('point_features_fwd', (coords, f32), (rois_xy5, f32), (fmap, f32), (coarse, f32))
    N, H, W, C = fmap.shape
    out = _empty((rows, 1, P, int(cin_p)), fmap.device)
    check(lib().mrcnn_point_features_fwd(ptr(coords), ptr(rois_xy5), ptr(fmap), N, H, W, C, float(scale), ptr(coarse), coarse.shape[1],
                                         coarse.shape[3], int(n_channels), rows, P, int(cin_p), ptr(out), stream_ptr()))
    return out


def point_features_bwd(g_in, coords, rois_xy5, scale, g_map):
    """g_map (N,H,W,C) += the fine part g_in (rows,1,P,ld)[..., :C] scattered by point_sample's transpose, in place and in a fixed order
    (mrcnn_point_features_bwd); returns g_map."""
    _ck(g_in, coords, rois_xy5, g_map)
    rows, P = coords.shape[0], coords.shape[1]
    if g_in.numel() != rows * P * g_in.shape[-1] or tuple(rois_xy5.shape) != (rows, 5) or g_map.dim() != 4:
        raise ValueError('point_features_bwd: g_in %r, coords %r, rois_xy5 %r, g_map %r' % (tuple(g_in.shape), tuple(coords.shape),
                                                                                           tuple(rois_xy5.shape), tuple(g_map.shape)))
    _point_dtypes('point_features_bwd', (g_in, f32), (coords, f32), (rois_xy5, f32), (g_map, f32))
    N, H, W, C = g_map.shape
    check(lib().mrcnn_point_features_bwd(ptr(g_in), g_in.shape[-1], ptr(coords), ptr(rois_xy5), rows, P, float(scale), ptr(g_map), N, H, W, C,
                                         stream_ptr()))
    return g_map


def point_concat_fwd(h, x0, c0, n_coarse, cin_p):
    """[h (..., Ch) | x0 (..., ld0)[..., c0 : c0 + n_coarse] | zeros] -> (..., cin_p) (mrcnn_point_concat_fwd)."""
    _ck(h, x0)
    n = h.numel() // h.shape[-1]
    if x0.numel() != n * x0.shape[-1]:
        raise ValueError('point_concat_fwd: h %r against x0 %r' % (tuple(h.shape), tuple(x0.shape)))
    _point_dtypes('point_concat_fwd', (h, f32), (x0, f32))
    out = _empty(tuple(h.shape[:-1]) + (int(cin_p),), h.device)
    check(lib().mrcnn_point_concat_fwd(ptr(h), h.shape[-1], ptr(x0), x0.shape[-1], int(c0), int(n_coarse), n, int(cin_p), ptr(out), stream_ptr()))
    return out


def point_concat_bwd(g_in, Ch):
    """g_in (..., cin_p)[..., :Ch] as a tensor of its own (mrcnn_point_concat_bwd): the coarse part is dropped."""
    _ck(g_in)
    _point_dtypes('point_concat_bwd', (g_in, f32))
    out = _empty(tuple(g_in.shape[:-1]) + (int(Ch),), g_in.device)
    check(lib().mrcnn_point_concat_bwd(ptr(g_in), g_in.shape[-1], int(Ch), g_in.numel() // g_in.shape[-1], ptr(out), stream_ptr()))
    return out


def point_target(masks, n_gt, rois_xy5, gt_assign, label, n_pos, n_sample, rows, coords):
    """Soft targets (mrcnn_point_target): masks (N,G,H,W) u8, the sampler's gt_assign (N*n_sample,) / n_pos (N,), the mask block's rois_xy5
    (N*rows,5) / label (N*rows,), coords (N*rows,P,2) -> (N*rows,P) in [0,1], -1 in the rows that are not live."""
    _ck(masks, n_gt, rois_xy5, gt_assign, label, n_pos, coords)
    if masks.dim() != 4 or masks.dtype != torch.uint8:
        raise ValueError('point_target: masks are an (N,G,H,W) uint8 tensor')
    N, G, H, W = masks.shape
    rows, n_sample = int(rows), int(n_sample)
    Rm = N * rows
    if coords.dim() != 3 or coords.shape[0] != Rm or coords.shape[2] != 2 or tuple(rois_xy5.shape) != (Rm, 5) or label.numel() != Rm \
            or gt_assign.numel() != N * n_sample or n_pos.numel() != N or n_gt.numel() != N:
        raise ValueError('point_target: the row counts of coords / rois_xy5 / label / gt_assign / n_pos / n_gt do not fit N = %d, n_sample = %d, '
                         'rows = %d' % (N, n_sample, rows))
    _point_dtypes('point_target', (n_gt, i32), (gt_assign, i32), (label, i32), (n_pos, i32), (rois_xy5, f32), (coords, f32))
    P = coords.shape[1]
    out = _empty((Rm, P), masks.device)
    check(lib().mrcnn_point_target(ptr(masks), N, G, H, W, ptr(n_gt), ptr(rois_xy5), ptr(gt_assign), ptr(label), ptr(n_pos), n_sample, rows,
                                   ptr(coords), P, ptr(out), stream_ptr()))
    return out


def point_bce(pred, target, label, n_channels, weight=1.0, label_base=1, want_grad=True, gx=None, out=None):
    """The point loss (mrcnn_point_bce): pred (rows,1,P,ld) or (rows*P,ld), target (rows,P) with -1 = skipped, label (rows,) i32 -> (out (2,)
    = (weight * mean BCE with logits over the live points, their count), gx shaped like pred)."""
    _ck(pred, target, label, gx)
    rows, P = target.shape
    ld = pred.shape[-1]
    if pred.numel() != rows * P * ld or label.numel() != rows:
        raise ValueError('point_bce: pred %r, target %r, %d labels' % (tuple(pred.shape), tuple(target.shape), label.numel()))
    _point_dtypes('point_bce', (pred, f32), (target, f32), (label, i32))
    out = _empty((2,), pred.device) if out is None else out
    if want_grad and gx is None:
        gx = torch.empty_like(pred)
    ws = _loss_ws(pred.device)
    check(lib().mrcnn_point_bce(ptr(pred), ld, int(n_channels), ptr(target), ptr(label), int(label_base), rows, P, float(weight), ptr(out),
                                ptr(gx) if want_grad else None, ptr(ws), ws.numel(), stream_ptr()))
    return out, gx


def point_subdivide(grid, label, n_channels, n_points):
    """One subdivision step's selection (mrcnn_point_subdivide): grid (D,S,S,ld) logits, label (D,) i32 0-based or None (channel 0) ->
    (up (D,2S,2S), index (D,n_sel) i32 ascending flat cells, coords (D,n_sel,2) their centres), n_sel = min(n_points, 4 S^2)."""
    _ck(grid, label)
    if grid.dim() != 4 or grid.shape[1] != grid.shape[2] or (label is not None and label.numel() != grid.shape[0]):
        raise ValueError('point_subdivide: grid %r' % (tuple(grid.shape),))
    _point_dtypes('point_subdivide', (grid, f32), (label, i32))
    D, S, _, ld = grid.shape
    n_sel = min(int(n_points), 4 * S * S)
    up = _empty((D, 2 * S, 2 * S), grid.device)
    index = _empty((D, max(n_sel, 0)), grid.device, i32)
    coords = _empty((D, max(n_sel, 0), 2), grid.device)
    check(lib().mrcnn_point_subdivide(ptr(grid), D, S, ld, int(n_channels), ptr(label), n_sel, ptr(up), ptr(index), ptr(coords), stream_ptr()))
    return up, index, coords


def point_scatter(pred, label, index, n_channels, grid):
    """grid (D,G,G)[d].flat[index[d, j]] = pred (D,1,n_sel,ld)[d, 0, j, label[d]] in place (mrcnn_point_scatter); returns grid."""
    _ck(pred, label, index, grid)
    D, n_sel = index.shape
    ld = pred.shape[-1]
    if pred.numel() != D * n_sel * ld or grid.shape[0] != D or (label is not None and label.numel() != D):
        raise ValueError('point_scatter: pred %r, index %r, grid %r' % (tuple(pred.shape), tuple(index.shape), tuple(grid.shape)))
    _point_dtypes('point_scatter', (pred, f32), (label, i32), (index, i32), (grid, f32))
    check(lib().mrcnn_point_scatter(ptr(pred), ld, int(n_channels), ptr(label), ptr(index), D, n_sel, int(np.prod(grid.shape[1:])), ptr(grid),
                                    stream_ptr()))
    return grid


def class_nms(cls_bbox, prob, l_begin, l_end, score_thresh, nms_thresh):
    """-> keep_idx (n_class,R) int32, keep_cnt (n_class,) int32."""
    _ck(cls_bbox, prob)
    R, n_class = prob.shape
    keep_idx = torch.full((n_class, max(R, 1)), -1, dtype=i32, device=prob.device)
    keep_cnt = torch.zeros((n_class,), dtype=i32, device=prob.device)
    if R > 0:
        check(lib().mrcnn_class_nms_f32(ptr(cls_bbox), ptr(prob), R, n_class, l_begin, l_end, float(score_thresh),
                                        float(nms_thresh), ptr(keep_idx), ptr(keep_cnt), stream_ptr()))
    return keep_idx, keep_cnt


def mask_paste(mask_logits, label, bbox, size):
    """mask_logits (D,S,S,Cm) NHWC, label (D,) int32, bbox (D,4) -> (D,H,W) uint8."""
    _ck(mask_logits, label, bbox)
    D, S, _, Cm = mask_logits.shape
    out = torch.empty((D, size[0], size[1]), dtype=torch.uint8, device=mask_logits.device)
    check(lib().mrcnn_mask_paste_f32(ptr(mask_logits), D, S, Cm, ptr(label), ptr(bbox), size[0], size[1], ptr(out),
                                     stream_ptr()))
    return out


def mask_iou_counts(a, b, a_label=None, b_label=None):
    """Exact overlap counts of two mask sets: a (Da,H,W) or (Da,HW), b (Db,...) bool / uint8 device tensors (any nonzero byte is a set
    pixel).  Returns (inter (Da,Db), area_a (Da,), area_b (Db,)) int32 on the device.  With labels ((Da,), (Db,) integer tensors, both
    or neither), pairs of different labels get inter 0 and cost no word work.  The bit-packed masks live in a workspace of this call."""
    if (a_label is None) != (b_label is None):
        raise ValueError('mask_iou_counts: give both label arrays or neither')
    _hip.require_cuda(a, b, a_label, b_label)
    if a.dim() < 1 or b.dim() < 1 or a.shape[1:] != b.shape[1:]:
        raise ValueError('mask_iou_counts: masks of different sizes %s and %s' % (tuple(a.shape), tuple(b.shape)))
    if a.dtype not in (torch.bool, torch.uint8) or b.dtype not in (torch.bool, torch.uint8):
        raise TypeError('mask_iou_counts: bool or uint8 masks expected, got %s and %s' % (a.dtype, b.dtype))
    Da, Db = a.shape[0], b.shape[0]
    HW = 1
    for s in a.shape[1:]:
        HW *= int(s)
    if HW > 0x7FFFFFFF:
        raise ValueError('mask_iou_counts: %d pixels per mask > 2^31 - 1' % HW)
    dev = a.device
    a = a.contiguous().view(torch.uint8)
    b = b.contiguous().view(torch.uint8)
    if a_label is not None and Da and Db:
        a_label = a_label.to(i32).contiguous()
        b_label = b_label.to(i32).contiguous()
    else:                       # labels change nothing when one side is empty
        a_label = b_label = None
    inter = torch.empty((Da, Db), dtype=i32, device=dev)
    area_a = torch.empty((Da,), dtype=i32, device=dev)
    area_b = torch.empty((Db,), dtype=i32, device=dev)
    nb = lib().mrcnn_mask_iou_workspace_bytes(Da, Db, HW)
    ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device=dev)
    check(lib().mrcnn_mask_iou_counts_u8(ptr(a), Da, ptr(a_label), ptr(b), Db, ptr(b_label), HW, ptr(ws), nb, ptr(inter), ptr(area_a),
                                         ptr(area_b), stream_ptr()))
    return inter, area_a, area_b


BOUNDARY_MAX_DILATION = 63      # csrc/evaluate.hip kMaxDilation: a horizontal shift stays within the neighbouring word
BOUNDARY_BAND_ROWS = 64         # csrc/evaluate.hip kBandRows: image rows of one tile of the boundary kernel
BOUNDARY_BAND_COLS = 8          # csrc/evaluate.hip kBandCols: 64-pixel word columns of one tile


def _boundary_args(who, masks, dilation):
    """(D, H, W, dilation) of (D,H,W) bool / uint8 masks; dilation None = evaluations.boundary_dilation(H, W)."""
    for m in masks:
        if m.dim() != 3:
            raise ValueError('%s: (D,H,W) masks expected, got %s' % (who, tuple(m.shape)))
        if m.dtype not in (torch.bool, torch.uint8):
            raise TypeError('%s: bool or uint8 masks expected, got %s' % (who, m.dtype))
    H, W = int(masks[0].shape[1]), int(masks[0].shape[2])
    if H * W > 0x7FFFFFFF:
        raise ValueError('%s: %d pixels per mask > 2^31 - 1' % (who, H * W))
    if dilation is None:
        from chainer_maskrcnn.evaluations import boundary_dilation
        dilation = boundary_dilation(H, W)
    if isinstance(dilation, bool) or int(dilation) != dilation or not 1 <= dilation <= BOUNDARY_MAX_DILATION:
        raise ValueError('%s: dilation must be an integer in 1..%d, got %r' % (who, BOUNDARY_MAX_DILATION, dilation))
    return H, W, int(dilation)


def mask_boundary_iou_counts(a, b, a_label=None, b_label=None, dilation=None):
    """Mask and boundary-band overlap counts of two mask sets (Boundary IoU, Cheng et al. 2021): a (Da,H,W), b (Db,H,W) bool / uint8
    device tensors (any nonzero byte is a set pixel).  The band of a mask M is M & ~erode(M, dilation), the erosion by a 3 x 3 block of
    ones with the outside of the image as background; dilation None = evaluations.boundary_dilation(H, W), else 1..63.  Returns (inter
    (Da,Db), area_a (Da,), area_b (Db,), binter (Da,Db), barea_a (Da,), barea_b (Db,)) int32 on the device: the first three are
    mask_iou_counts', the last three the same counts of the bands.  Labels as in mask_iou_counts."""
    if (a_label is None) != (b_label is None):
        raise ValueError('mask_boundary_iou_counts: give both label arrays or neither')
    _hip.require_cuda(a, b, a_label, b_label)
    if a.dim() != 3 or b.dim() != 3 or a.shape[1:] != b.shape[1:]:
        raise ValueError('mask_boundary_iou_counts: (D,H,W) masks of one size expected, got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    H, W, dilation = _boundary_args('mask_boundary_iou_counts', (a, b), dilation)
    Da, Db = a.shape[0], b.shape[0]
    dev = a.device
    a = a.contiguous().view(torch.uint8)
    b = b.contiguous().view(torch.uint8)
    if a_label is not None and Da and Db:
        a_label = a_label.to(i32).contiguous()
        b_label = b_label.to(i32).contiguous()
    else:                       # labels change nothing when one side is empty
        a_label = b_label = None
    out = [torch.empty(s, dtype=i32, device=dev) for s in ((Da, Db), (Da,), (Db,)) * 2]
    nb = lib().mrcnn_mask_boundary_workspace_bytes(Da, Db, H, W)
    ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device=dev)
    check(lib().mrcnn_mask_boundary_iou_counts_u8(ptr(a), Da, ptr(a_label), ptr(b), Db, ptr(b_label), H, W, dilation, ptr(ws), nb,
                                                  *[ptr(o) for o in out], stream_ptr()))
    return tuple(out)


def mask_boundary_words(masks, dilation=None):
    """The boundary bands of masks (D,H,W) bool / uint8 (the first stage of mask_boundary_iou_counts) as bit-packed rows: (D, H,
    ceil(W/64)) int64 on the device, bit k of word w of a row = band pixel 64 w + k, tail bits zero."""
    _hip.require_cuda(masks)
    H, W, dilation = _boundary_args('mask_boundary_words', (masks,), dilation)
    D = masks.shape[0]
    masks = masks.contiguous().view(torch.uint8)
    out = torch.empty((D, H, (W + 63) // 64), dtype=torch.int64, device=masks.device)
    nb = lib().mrcnn_mask_boundary_workspace_bytes(D, 0, H, W)
    ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device=masks.device)
    check(lib().mrcnn_mask_boundary_words_u8(ptr(masks), D, H, W, dilation, ptr(ws), nb, ptr(out), stream_ptr()))
    return out


def keypoint_decode(heat, bbox, K, return_index=False):
    """Keypoints from the keypoint branch's heat maps: heat (D,S,S,Cp) float32 NHWC (FPNRoIMaskHead.mask_branch of the keypoint head,
    Cp = pad32(K)), bbox (D,4) float32 (y1,x1,y2,x2) in image coordinates.  Returns (D,K,4) float32 (y, x, logit, prob) on the device:
    the first argmax over the S*S cells of channel k, the top-left corner of that cell mapped into the box, its logit and the softmax
    probability over the cells there (include/mrcnn_hip.h, mrcnn_keypoint_decode_f32); with return_index also the (D,K) int32 flat
    argmax cy * S + cx."""
    _hip.require_cuda(heat, bbox)
    if heat.dim() != 4 or heat.shape[1] != heat.shape[2]:
        raise ValueError('keypoint_decode: heat maps (D,S,S,Cp) expected, got %s' % (tuple(heat.shape),))
    if heat.dtype != f32 or bbox.dtype != f32:
        raise TypeError('keypoint_decode: float32 heat maps and boxes expected, got %s and %s' % (heat.dtype, bbox.dtype))
    D, S, Cp = heat.shape[0], heat.shape[1], heat.shape[3]
    if not 0 < K <= Cp or Cp % 4:
        raise ValueError('keypoint_decode: K %d against %d channels (a multiple of 4, >= K, is needed)' % (K, Cp))
    if tuple(bbox.shape) != (D, 4):
        raise ValueError('keypoint_decode: boxes (%d,4) expected, got %s' % (D, tuple(bbox.shape)))
    heat, bbox = heat.contiguous(), bbox.contiguous()
    if heat.data_ptr() % 16:                    # a view into its storage: the kernel reads 16-byte cells
        heat = heat.clone()
    out = _empty((D, K, 4), heat.device)
    idx = _empty((D, K), heat.device, i32) if return_index else None
    if D:
        nb = lib().mrcnn_keypoint_decode_workspace_bytes(D, S, K)
        ws = torch.empty((nb,), dtype=torch.uint8, device=heat.device)
        check(lib().mrcnn_keypoint_decode_f32(ptr(heat), D, S, Cp, K, ptr(bbox), ptr(ws), nb, ptr(out), ptr(idx), stream_ptr()))
    return (out, idx) if return_index else out


def mask_rle_encode(masks):
    """COCO run-length codes of masks (D,H,W) bool / uint8 device tensor (any nonzero byte is a set pixel; rows may start at any byte
    offset): runs over the column-major flattening, starting with a run of 0s (maskApi.c rleEncode).  Returns (offsets (D+1,),
    counts (offsets[D],), area (D,)) int32 on the device: mask d's runs are counts[offsets[d]:offsets[d+1]], area its set pixels.
    One device->host read, of offsets[D], sizes counts."""
    _hip.require_cuda(masks)
    if masks.dim() != 3:
        raise ValueError('mask_rle_encode: masks (D,H,W) expected, got %s' % (tuple(masks.shape),))
    if masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError('mask_rle_encode: bool or uint8 masks expected, got %s' % masks.dtype)
    D, H, W = (int(s) for s in masks.shape)
    if H * W > 0x7FFFFFFF or D * (H * W + 1) > 0x7FFFFFFF:
        raise ValueError('mask_rle_encode: %d masks of %d x %d pixels: the run total may not fit int32' % (D, H, W))
    dev = masks.device
    m = masks.contiguous().view(torch.uint8)
    offsets = torch.empty((D + 1,), dtype=i32, device=dev)
    area = torch.empty((D,), dtype=i32, device=dev)
    nb = lib().mrcnn_mask_rle_workspace_bytes(D, H, W)
    ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device=dev)
    check(lib().mrcnn_mask_rle_count_u8(ptr(m), D, H, W, ptr(ws), nb, ptr(offsets), ptr(area), stream_ptr()))
    n = int(offsets[D].item()) if D else 0                 # the one device->host read: the size of counts
    counts = torch.empty((n,), dtype=i32, device=dev)
    if D:
        check(lib().mrcnn_mask_rle_write_u8(ptr(m), D, H, W, ptr(ws), nb, ptr(offsets), ptr(counts), stream_ptr()))
    return offsets, counts, area


# ---- test-time augmentation (tta.hip) -----------------------------------------------------------------------------------------------------
# mrcnn_tta_view_t of include/mrcnn_hip.h, one row per view
TTA_VIEW = np.dtype([('R', '<i4'), ('mirror', '<i4'), ('scale', '<f4')])
assert TTA_VIEW.itemsize == 12
TTA_VIEWS_MAX = 8
CLASS_NMS_WS_MAX = 4096


def tta_views(rows):
    """[(R, mirror, scale)] -> the host view table the TTA calls take."""
    return np.array([(int(r), int(m), float(s)) for r, m, s in rows], TTA_VIEW)


def _dev_ptrs(ts):
    """A host array of device pointers (NULL for None / empty tensors); kept alive by the caller for the call."""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None and t.numel() else None for t in ts])


def image_resize_mirror_f32(img, oh, ow, mirror, div=1.0):
    """img (C,H,W) float32 -> (C,oh,ow): image_resize_f32 of img, or of img.flip(-1) with mirror=1 (same bits), then / div."""
    _ck(img)
    C, H, W = img.shape
    out = _empty((C, oh, ow), img.device)
    check(lib().mrcnn_image_resize_mirror_f32(ptr(img), C, H, W, ptr(out), oh, ow, oh, ow, int(mirror), float(div), stream_ptr()))
    return out


def tta_detect_decode(rois, box_outs, mirrors, scales, n_class, loc0, mean, std, size):
    """Per view v: rois[v] (R_v,4), box_outs[v] (R_v,ld), mirror, scale.  Returns the union cls_bbox (R,4), prob (R,n_class), rows in view
    order: detect_decode of each view with its scale, a mirrored view's boxes mapped back to (y1, W-x2, y2, W-x1).  One launch."""
    _ck(*rois)
    _ck(*box_outs)
    V = len(rois)
    if not (len(box_outs) == len(mirrors) == len(scales) == V):
        raise ValueError('tta_detect_decode: %d views of rois against %d / %d / %d' % (V, len(box_outs), len(mirrors), len(scales)))
    ld = box_outs[0].shape[1]
    if any(b.dim() != 2 or b.shape[1] != ld or b.shape[0] != r.shape[0] for r, b in zip(rois, box_outs)):
        raise ValueError('tta_detect_decode: box outputs (R_v, %d) matching the rois expected' % ld)
    views = tta_views([(r.shape[0], m, s) for r, m, s in zip(rois, mirrors, scales)])
    R = int(views['R'].sum())
    dev = rois[0].device
    cls_bbox, prob = _empty((R, 4), dev), _empty((R, n_class), dev)
    pr, pb = _dev_ptrs(rois), _dev_ptrs(box_outs)
    m4 = (ctypes.c_float * 4)(*mean)
    s4 = (ctypes.c_float * 4)(*std)
    check(lib().mrcnn_tta_detect_decode_f32(ctypes.cast(pr, ctypes.c_void_p), ctypes.cast(pb, ctypes.c_void_p), views.ctypes.data, V, ld,
                                            n_class, loc0, ctypes.cast(m4, ctypes.c_void_p), ctypes.cast(s4, ctypes.c_void_p),
                                            float(size[0]), float(size[1]), ptr(cls_bbox), ptr(prob), stream_ptr()))
    return cls_bbox, prob


def class_nms_ws(cls_bbox, prob, l_begin, l_end, score_thresh, nms_thresh):
    """class_nms for up to 4096 candidates (the union of the TTA views) -> keep_idx (n_class,R) int32, keep_cnt (n_class,) int32; the
    same keep lists.  R <= 512 runs class_nms's kernel; above, the sorted candidates and the IoU bitmask live in a workspace of this call."""
    _ck(cls_bbox, prob)
    R, n_class = prob.shape
    keep_idx = torch.full((n_class, max(R, 1)), -1, dtype=i32, device=prob.device)
    keep_cnt = torch.zeros((n_class,), dtype=i32, device=prob.device)
    if R > 0:
        nb = lib().mrcnn_class_nms_workspace_bytes(R, n_class)
        ws = torch.empty((nb,), dtype=torch.uint8, device=prob.device) if nb else None
        check(lib().mrcnn_class_nms_ws_f32(ptr(cls_bbox), ptr(prob), R, n_class, l_begin, l_end, float(score_thresh), float(nms_thresh),
                                           ptr(keep_idx), ptr(keep_cnt), ptr(ws), nb, stream_ptr()))
    return keep_idx, keep_cnt


SOFT_NMS_METHODS = {'hard': 0, 'linear': 1, 'gaussian': 2}       # MRCNN_SOFT_NMS_* of include/mrcnn_hip.h
BOXPOST_MAX = 4096                                                # MRCNN_BOXPOST_MAX


def class_soft_nms(cls_bbox, prob, l_begin, l_end, score_thresh, method, nms_thresh, sigma):
    """Soft-NMS per class (mrcnn_class_soft_nms_f32) for up to 4096 candidates -> keep_idx (n_class,R) int32, keep_score
    (n_class,R) float32 (the decayed scores, in selection order), keep_cnt (n_class,) int32.  method: 'hard' (class_nms's keep lists),
    'linear' or 'gaussian'."""
    if method not in SOFT_NMS_METHODS:
        raise ValueError('class_soft_nms: method must be one of %s, got %r' % (sorted(SOFT_NMS_METHODS), method))
    _ck(cls_bbox, prob)
    R, n_class = prob.shape
    keep_idx = torch.full((n_class, max(R, 1)), -1, dtype=i32, device=prob.device)
    keep_score = torch.zeros((n_class, max(R, 1)), dtype=torch.float32, device=prob.device)
    keep_cnt = torch.zeros((n_class,), dtype=i32, device=prob.device)
    if R > 0:
        nb = lib().mrcnn_class_soft_nms_workspace_bytes(R, n_class)
        ws = torch.empty((nb,), dtype=torch.uint8, device=prob.device) if nb else None
        check(lib().mrcnn_class_soft_nms_f32(ptr(cls_bbox), ptr(prob), R, n_class, l_begin, l_end, float(score_thresh),
                                             SOFT_NMS_METHODS[method], float(nms_thresh), float(sigma), ptr(keep_idx), ptr(keep_score),
                                             ptr(keep_cnt), ptr(ws), nb, stream_ptr()))
    return keep_idx, keep_score, keep_cnt


def box_vote(cls_bbox, prob, l_begin, l_end, score_thresh, vote_thresh, keep_idx, keep_cnt, out=None):
    """Box voting (mrcnn_box_vote_f32): keep_box (n_class,R,4) float32, row [l,k] = the prob-weighted mean of the boxes
    of class l's candidates whose IoU with the kept box keep_idx[l,k] is >= vote_thresh, for k < keep_cnt[l]; the other rows are not
    written (zeros, or what ``out`` held)."""
    _ck(cls_bbox, prob, keep_idx, keep_cnt)
    R, n_class = prob.shape
    if tuple(keep_idx.shape) != (n_class, max(R, 1)) or tuple(keep_cnt.shape) != (n_class,) or keep_idx.dtype != i32 or keep_cnt.dtype != i32:
        raise ValueError('box_vote: keep_idx (%d,%d) / keep_cnt (%d,) int32 expected, got %s %s / %s %s'
                         % (n_class, max(R, 1), n_class, tuple(keep_idx.shape), keep_idx.dtype, tuple(keep_cnt.shape), keep_cnt.dtype))
    if out is None:
        out = torch.zeros((n_class, max(R, 1), 4), dtype=torch.float32, device=prob.device)
    else:
        _ck(out)
        if tuple(out.shape) != (n_class, max(R, 1), 4) or out.dtype != torch.float32:
            raise ValueError('box_vote: out (%d,%d,4) float32 expected, got %s %s' % (n_class, max(R, 1), tuple(out.shape), out.dtype))
    if R > 0:
        check(lib().mrcnn_box_vote_f32(ptr(cls_bbox), ptr(prob), R, n_class, l_begin, l_end, float(score_thresh), float(vote_thresh),
                                       ptr(keep_idx), ptr(keep_cnt), ptr(out), stream_ptr()))
    return out


def tta_mask_merge(mask_logits, mirrors, label):
    """mask_logits: per view (D,S,S,Cm) NHWC; label (D,) int32.  Returns prob (D,S,S) float32 = the mean over the views, in order, of
    sigmoid(logit) of channel label[d], read at column S-1-x in a mirrored view."""
    _ck(*mask_logits)
    _ck(label)
    V = len(mask_logits)
    if len(mirrors) != V:
        raise ValueError('tta_mask_merge: %d views of logits against %d mirror flags' % (V, len(mirrors)))
    shape = tuple(mask_logits[0].shape)
    if len(shape) != 4 or shape[1] != shape[2] or any(tuple(m.shape) != shape for m in mask_logits):
        raise ValueError('tta_mask_merge: (D,S,S,Cm) logits of one shape expected, got %s' % [tuple(m.shape) for m in mask_logits])
    D, S, _, Cm = shape
    views = tta_views([(0, m, 1.0) for m in mirrors])
    out = _empty((D, S, S), label.device)
    p = _dev_ptrs(mask_logits)
    check(lib().mrcnn_tta_mask_merge_f32(ctypes.cast(p, ctypes.c_void_p), views.ctypes.data, V, D, S, Cm, ptr(label), ptr(out),
                                         stream_ptr()))
    return out


def mask_paste_prob(prob, bbox, size):
    """prob (D,S,S) float32, bbox (D,4) -> (D,H,W) uint8: mask_paste's resize, threshold and paste rule from probabilities."""
    _ck(prob, bbox)
    D, S = prob.shape[0], prob.shape[1]
    out = torch.empty((D, size[0], size[1]), dtype=torch.uint8, device=prob.device)
    check(lib().mrcnn_mask_paste_prob_f32(ptr(prob), D, S, ptr(bbox), size[0], size[1], ptr(out), stream_ptr()))
    return out


def tta_keypoint_merge(heat, mirrors, K, perm=None):
    """heat: per view (D,S,S,Cp) NHWC heat maps.  Returns (D,S,S,Cp) float32 = the mean over the views, in order, of heat[u][d, y, x_u, k_u]:
    x_u = S-1-x and k_u = perm[k] (k < K) in a mirrored view.  perm: K ints, needed when a view is mirrored."""
    _ck(*heat)
    V = len(heat)
    if len(mirrors) != V:
        raise ValueError('tta_keypoint_merge: %d views of heat maps against %d mirror flags' % (V, len(mirrors)))
    shape = tuple(heat[0].shape)
    if len(shape) != 4 or shape[1] != shape[2] or any(tuple(h.shape) != shape for h in heat):
        raise ValueError('tta_keypoint_merge: (D,S,S,Cp) heat maps of one shape expected, got %s' % [tuple(h.shape) for h in heat])
    D, S, _, Cp = shape
    views = tta_views([(0, m, 1.0) for m in mirrors])
    pa = None
    if perm is not None:
        pa = np.ascontiguousarray(perm, np.int32)
        if pa.shape != (K,):
            raise ValueError('tta_keypoint_merge: a permutation of %d channels expected, got %d' % (K, pa.size))
    out = _empty(shape, heat[0].device)
    p = _dev_ptrs(heat)
    check(lib().mrcnn_tta_keypoint_merge_f32(ctypes.cast(p, ctypes.c_void_p), views.ctypes.data, V, D, S, Cp, K,
                                             pa.ctypes.data if pa is not None else None, ptr(out), stream_ptr()))
    return out


# ---- rendering of detections (vis.hip) ------------------------------------------------------------------------------------------------
# mrcnn_vis_prim_t of include/mrcnn_hip.h, one row per primitive; rgb = r | g << 8 | b << 16
VIS_PRIM = np.dtype([(k, '<i4') for k in ('kind', 'x0', 'y0', 'x1', 'y1', 'p', 'rgb', 'a')])
assert VIS_PRIM.itemsize == 32
VIS_RECT, VIS_SEGMENT, VIS_DISC, VIS_GLYPH, VIS_FILL = range(5)
VIS_DRAW_MASKS, VIS_DRAW_CONTOURS, VIS_DRAW_BOXES = 1, 2, 4
VIS_MAX_SIDE, VIS_COORD_MIN, VIS_COORD_MAX, VIS_PARAM_MAX, VIS_GLYPH_SCALE_MAX, VIS_GLYPHS_MAX = 16384, -4096, 20479, 4096, 64, 256


def check_vis_prims(prims):
    """The primitive array as VIS_PRIM rows, every cap of include/mrcnn_hip.h checked on the host (the kernel cannot report a bad
    descriptor; it would draw nothing for it).  ValueError names the first offending row."""
    p = np.ascontiguousarray(prims)
    if p.dtype != VIS_PRIM:
        if p.dtype != np.int32 or p.ndim != 2 or p.shape[1] != 8:
            raise ValueError('vis primitives: a VIS_PRIM array or (P,8) int32 expected, got %s %s' % (p.dtype, p.shape))
        p = p.view(VIS_PRIM).reshape(-1)
    if p.ndim != 1:
        raise ValueError('vis primitives: a flat VIS_PRIM array expected, got shape %s' % (p.shape,))
    kind, two = p['kind'], np.isin(p['kind'], (VIS_RECT, VIS_SEGMENT, VIS_FILL))
    p_min = np.select([kind == VIS_DISC, kind == VIS_FILL], [0, 0], 1)
    p_max = np.where(kind == VIS_GLYPH, VIS_GLYPH_SCALE_MAX, VIS_PARAM_MAX)
    bad = (kind < 0) | (kind > VIS_FILL) | (p['a'] < 0) | (p['a'] > 256) | (p['p'] < p_min) | (p['p'] > p_max)
    bad |= (p['rgb'] < 0) | (p['rgb'] > 0xFFFFFF)
    for k in ('x0', 'y0'):
        bad |= (p[k] < VIS_COORD_MIN) | (p[k] > VIS_COORD_MAX)
    for k in ('x1', 'y1'):
        bad |= two & ((p[k] < VIS_COORD_MIN) | (p[k] > VIS_COORD_MAX))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError('vis primitives: row %d %s breaks a cap (coordinates %d..%d, p <= %d, glyph scale 1..%d, a 0..256, kind 0..4)'
                         % (i, p[i], VIS_COORD_MIN, VIS_COORD_MAX, VIS_PARAM_MAX, VIS_GLYPH_SCALE_MAX))
    return p


def vis_render(img, masks=None, bbox=None, colors=None, order=None, mask_a256=128, box_thickness=1, flags=0, prims=None, font=None):
    """img (3,H,W) float32 device tensor (RGB 0..255) -> (H,W,3) uint8 device tensor, drawn by mrcnn_vis_render_u8 (its contract: include/
    mrcnn_hip.h).  masks (D,H,W) bool / uint8 and bbox (D,4) float32 on the device (None when not drawn), colors (D,3) uint8 (host array or
    device tensor), order a host array of D instance indices (the drawing order; None: 0..D-1), prims a host VIS_PRIM array, font a host array of uint64 glyph bitmaps.  One launch; the only copies are the small
    host->device uploads of colors, prims and font."""
    _hip.require_cuda(img)
    if img.dim() != 3 or img.shape[0] != 3 or img.dtype != f32:
        raise ValueError('vis_render: a (3,H,W) float32 image expected, got %s %s' % (tuple(img.shape), img.dtype))
    H, W = int(img.shape[1]), int(img.shape[2])
    if H > VIS_MAX_SIDE or W > VIS_MAX_SIDE:
        raise ValueError('vis_render: image %d x %d larger than %d a side' % (H, W, VIS_MAX_SIDE))
    dev = img.device
    img = img.contiguous()
    D = 0
    for name, t, tail in (('masks', masks, (H, W)), ('bbox', bbox, (4,)), ('colors', colors, (3,))):
        if t is not None:
            if tuple(t.shape[1:]) != tail or t.ndim != len(tail) + 1:
                raise ValueError('vis_render: %s (D,%s) expected, got %s' % (name, ','.join(str(s) for s in tail), tuple(t.shape)))
            D = max(D, int(t.shape[0]))
    for name, t in (('masks', masks), ('bbox', bbox), ('colors', colors)):
        if t is not None and int(t.shape[0]) != D:
            raise ValueError('vis_render: %s has %d instances, another argument %d' % (name, int(t.shape[0]), D))
    if D and colors is None:
        raise ValueError('vis_render: colors (D,3) needed for %d instances' % D)
    if masks is not None:
        _hip.require_cuda(masks)
        if masks.dtype not in (torch.bool, torch.uint8):
            raise TypeError('vis_render: bool or uint8 masks expected, got %s' % masks.dtype)
        masks = masks.contiguous().view(torch.uint8)
    elif D and flags & (VIS_DRAW_MASKS | VIS_DRAW_CONTOURS):
        raise ValueError('vis_render: masks needed to draw masks or contours')
    if bbox is not None:
        _hip.require_cuda(bbox)
        bbox = bbox.to(f32).contiguous()
    elif D and flags & VIS_DRAW_BOXES:
        raise ValueError('vis_render: bbox needed to draw boxes')
    if colors is not None:
        if not isinstance(colors, torch.Tensor):
            colors = torch.from_numpy(np.ascontiguousarray(colors, np.uint8))
        if colors.dtype != torch.uint8:
            raise TypeError('vis_render: uint8 colors expected, got %s' % colors.dtype)
        colors = colors.to(dev).contiguous()
    order_d = None
    if order is not None and D:
        o = np.ascontiguousarray(order, np.int32).reshape(-1)
        if o.shape[0] != D or (o < 0).any() or (o >= D).any():
            raise ValueError('vis_render: order must hold %d indices in 0..%d' % (D, D - 1))
        order_d = torch.from_numpy(o).to(dev)
    pr = check_vis_prims(prims) if prims is not None and len(prims) else None
    prims_d = torch.from_numpy(pr.view(np.int32).reshape(-1, 8)).to(dev) if pr is not None else None
    ft = np.ascontiguousarray(font, np.uint64).reshape(-1) if font is not None and len(font) else None
    font_d = torch.from_numpy(ft.view(np.int64)).to(dev) if ft is not None else None
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    check(lib().mrcnn_vis_render_u8(ptr(img), H, W, ptr(masks), ptr(bbox), ptr(colors), ptr(order_d), D, int(mask_a256), int(box_thickness), int(flags),
                                    ptr(prims_d), 0 if pr is None else int(pr.shape[0]), ptr(font_d), 0 if ft is None else int(ft.shape[0]),
                                    ptr(out), stream_ptr()))
    return out


# ---- deformable convolution (csrc/deform.hip) --------------------------------------------------------------------------------
DEFORM_GEOMETRY = (3, 3, 1, 1, 1, 1)        # KH, KW, stride, pad, dilation, deformable groups: the one geometry the kernels take


def _deform_args(name, x_shape, off, ts):
    _ck(off, *ts)
    for t_ in (off,) + tuple(ts):
        if t_ is not None and t_.dtype != f32:
            raise ValueError('%s: a %s tensor where %s is expected' % (name, t_.dtype, f32))
    if len(x_shape) != 4 or off.dim() != 4 or tuple(off.shape[:3]) != tuple(x_shape[:3]):
        raise ValueError('%s: a map of shape %r against offsets %r' % (name, tuple(x_shape), tuple(off.shape)))


def deform_cols_fwd(x, off, modulated):
    """x (N,H,W,C), off (N,H,W,ld): (dy, dx) of tap k in channels 2k, 2k + 1, modulated the logit of its mask in channel 18 + k -> the sampled
    columns (N,H,W,9*C), tap-major (mrcnn_deform_cols_fwd_f32)."""
    _deform_args('deform_cols_fwd', x.shape, off, (x,))
    N, H, W, C = x.shape
    cols = _empty((N, H, W, 9 * C), x.device)
    check(lib().mrcnn_deform_cols_fwd_f32(ptr(x), ptr(off), off.shape[3], int(bool(modulated)), N, H, W, C, *DEFORM_GEOMETRY, ptr(cols),
                                          stream_ptr()))
    return cols


def deform_offset_bwd(g_cols, x, off, modulated):
    """The gradient of the whole offset row (N,H,W,ld) from g_cols (N,H,W,9*C): channels 2k, 2k + 1, modulated 18 + k, zeros behind them
    (mrcnn_deform_offset_bwd_f32)."""
    _deform_args('deform_offset_bwd', x.shape, off, (g_cols, x))
    N, H, W, C = x.shape
    if g_cols.numel() != 9 * x.numel():
        raise ValueError('deform_offset_bwd: g_cols %r against x %r' % (tuple(g_cols.shape), tuple(x.shape)))
    g_off = _empty(tuple(off.shape), x.device)
    check(lib().mrcnn_deform_offset_bwd_f32(ptr(g_cols), ptr(x), ptr(off), off.shape[3], int(bool(modulated)), N, H, W, C, *DEFORM_GEOMETRY,
                                            ptr(g_off), stream_ptr()))
    return g_off


def deform_input_bwd(g_cols, off, modulated, x_shape, gx=None, relu_x=None):
    """The gradient of x (N,H,W,C) from g_cols (N,H,W,9*C), the same bits on every run (mrcnn_deform_input_bwd_f32).  gx given: added into it,
    its prior value first; relu_x: the TOTAL is zeroed where relu_x <= 0.  Returns gx."""
    _deform_args('deform_input_bwd', x_shape, off, (g_cols, gx, relu_x))
    N, H, W, C = x_shape
    if g_cols.numel() != 9 * N * H * W * C or (gx is not None and tuple(gx.shape) != tuple(x_shape)) \
            or (relu_x is not None and tuple(relu_x.shape) != tuple(x_shape)):
        raise ValueError('deform_input_bwd: g_cols %r, gx %r, relu_x %r against a map of %r' % (
            tuple(g_cols.shape), None if gx is None else tuple(gx.shape), None if relu_x is None else tuple(relu_x.shape), tuple(x_shape)))
    acc = gx is not None
    if gx is None:
        gx = _empty(tuple(x_shape), g_cols.device)
    ws = workspace(lib().mrcnn_deform_input_bwd_workspace_bytes(N, H, W), g_cols.device)
    check(lib().mrcnn_deform_input_bwd_f32(ptr(g_cols), ptr(off), off.shape[3], int(bool(modulated)), N, H, W, C, *DEFORM_GEOMETRY, ptr(gx),
                                           ptr(relu_x), int(acc), ptr(ws), ws.numel(), stream_ptr()))
    return gx
