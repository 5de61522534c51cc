"""References of GroupNorm in the FPN (csrc/groupnorm_map.hip, nn/core.py MapGroupNorm, FeaturePyramidNetwork(fpn_norm='gn'); DESIGN.md
section 3.23).
  group_norm_fwd / group_norm_bwd   the float64 NumPy statement of tests/groupnorm_reference.py (no ReLU: the FPN has none), and with
                                    dtype=np.float32 the same computation carried out in float32 - its distance from the float64 result on
                                    the same data is the floor a float32 kernel is held against.
  top_down                          the top-down pyramid on torch CPU tensors in a chosen dtype, from F.conv2d, F.group_norm and
                                    oracle.model.upsample_add, with autograd for its backward."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import groupnorm_reference as gnr  # noqa: E402


def _grouped(t, C, G):
    R, H, W, _ = t.shape
    return t[..., :C].reshape(R, H * W, G, C // G)


def group_norm_fwd(x, gamma, beta, C, G, eps=1e-5, dtype=np.float64):
    """Returns (y (R,H,W,Cp), mean (R,G), rstd (R,G)) in ``dtype``; float64 is tests/groupnorm_reference.py itself."""
    if dtype == np.float64:
        return gnr.group_norm_fwd(x, gamma, beta, C, G, relu=False, eps=eps)
    D = dtype
    x, gamma, beta = np.asarray(x, D), np.asarray(gamma, D), np.asarray(beta, D)
    R, H, W, Cp = x.shape
    xg = _grouped(x, C, G)
    mean = xg.mean(axis=(1, 3), dtype=D)
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3), dtype=D)
    rstd = (D(1.0) / np.sqrt(var + D(eps))).astype(D)
    xh = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(R, H, W, C)
    y = np.zeros((R, H, W, Cp), D)
    y[..., :C] = gamma[:C] * xh + beta[:C]
    return y, mean, rstd


def group_norm_bwd(gy, x, gamma, mean, rstd, C, G, dtype=np.float64):
    """Returns (gx (R,H,W,Cp), ggamma (Cp,), gbeta (Cp,)) in ``dtype``."""
    if dtype == np.float64:
        return gnr.group_norm_bwd(gy, x, gamma, mean, rstd, C, G, mask=None)
    D = dtype
    gy, x, gamma, mean, rstd = (np.asarray(t, D) for t in (gy, x, gamma, mean, rstd))
    R, H, W, Cp = x.shape
    cpg = C // G
    dzg, xg = _grouped(gy, C, G), _grouped(x, C, G)
    xh = (xg - mean[:, None, :, None]) * rstd[:, None, :, None]
    gt = dzg * gamma[:C].reshape(1, 1, G, cpg)
    a = gt.mean(axis=(1, 3), keepdims=True, dtype=D)
    b = (gt * xh).mean(axis=(1, 3), keepdims=True, dtype=D)
    gx = np.zeros((R, H, W, Cp), D)
    gx[..., :C] = (rstd[:, None, :, None] * (gt - a - xh * b)).reshape(R, H, W, C)
    ggamma, gbeta = np.zeros((Cp,), D), np.zeros((Cp,), D)
    ggamma[:C] = (dzg * xh).sum(axis=(0, 1), dtype=D).reshape(C)
    gbeta[:C] = dzg.sum(axis=(0, 1), dtype=D).reshape(C)
    return gx, ggamma, gbeta


def all_six(x, gy, gamma, beta, C, G, dtype):
    """{'y', 'mean', 'rstd', 'gx', 'ggamma', 'gbeta'} of one forward and backward in ``dtype`` (the padding of x and gy zeroed first)."""
    x, gy = np.array(x, dtype), np.array(gy, dtype)
    x[..., C:] = 0
    gy[..., C:] = 0
    y, mean, rstd = group_norm_fwd(x, gamma, beta, C, G, dtype=dtype)
    gx, gg, gb = group_norm_bwd(gy, x, gamma, mean, rstd, C, G, dtype=dtype)
    return {'y': y, 'mean': mean, 'rstd': rstd, 'gx': gx, 'ggamma': gg, 'gbeta': gb}


FPN_CONVS = ('toplayer', 'lat_p4', 'lat_p3', 'lat_p2', 'conv_p4', 'conv_p3', 'conv_p2', 'conv_p6')


def top_down(P, cs, grads, groups, dtype):
    """P: {'<conv>/W' (Cout,k,k,Cin) in the store's layout, '<conv>/b', '<conv>/gn/gamma', '<conv>/gn/beta'} for the eight FPN_CONVS
    (logical channels only); cs = (c2, c3, c4, c5) and grads = the upstream gradients of (p2 .. p6), NHWC.  Returns
    ((p2 .. p6), (g_c2 .. g_c5), {name: parameter gradient}) in ``dtype``, NHWC / the store's layout."""
    from oracle.model import upsample_add
    leaves = {n: v.to(dtype).clone().requires_grad_(True) for n, v in P.items()}
    cs = [c.to(dtype).clone().requires_grad_(True) for c in cs]

    def layer(name, x, stride=1):
        w = leaves[name + '/W']
        h = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), leaves[name + '/b'], stride=stride, padding=w.shape[1] // 2)
        h = F.group_norm(h, groups, leaves[name + '/gn/gamma'], leaves[name + '/gn/beta'], eps=1e-5)
        return h.permute(0, 2, 3, 1)
    c2, c3, c4, c5 = cs
    p5 = layer('toplayer', c5)
    p4 = layer('conv_p4', upsample_add(p5, layer('lat_p4', c4)))
    p3 = layer('conv_p3', upsample_add(p4, layer('lat_p3', c3)))
    p2 = layer('conv_p2', upsample_add(p3, layer('lat_p2', c2)))
    p6 = layer('conv_p6', p5, stride=2)
    ps = (p2, p3, p4, p5, p6)
    sum((p * g.to(dtype)).sum() for p, g in zip(ps, grads)).backward()
    return tuple(p.detach() for p in ps), tuple(c.grad for c in cs), {n: v.grad for n, v in leaves.items()}
