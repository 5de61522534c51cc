"""Float64 NumPy statement of GroupNorm forward and backward (csrc/groupnorm.hip, gn_common.h), with the signature
conventions of ops.group_norm_fwd / ops.group_norm_bwd: NHWC (R, H, W, Cp), C logical channels in G groups of cpg = C / G, statistics per
(sample, group) over H * W * cpg elements, biased variance about the mean, eps 1e-5.  Padded channels c >= C give zeros everywhere.  The
ReLU mask of the backward is an INPUT (a boolean array shaped like x, or None), so a test can hand it the device's own y > 0 and a
sign flip at |y| ~ 0 decides nothing.  tests/test_groupnorm_cpu.py holds it against torch.nn.functional.group_norm in float64."""
import numpy as np

D = np.float64


def _grouped(t, C, G):
    R, H, W, _ = t.shape
    return t[..., :C].reshape(R, H * W, G, C // G)


def group_norm_fwd(x, gamma, beta, C, G, relu=False, eps=1e-5):
    """Returns (y (R,H,W,Cp), mean (R,G), rstd (R,G)) in float64."""
    x, gamma, beta = np.asarray(x, D), np.asarray(gamma, D), np.asarray(beta, D)
    R, H, W, Cp = x.shape
    xg = _grouped(x, C, G)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + eps)
    xh = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(R, H, W, C)
    y = np.zeros((R, H, W, Cp), D)
    y[..., :C] = gamma[:C] * xh + beta[:C]
    if relu:
        y = np.maximum(y, 0.0)
    return y, mean, rstd


def group_norm_bwd(gy, x, gamma, mean, rstd, C, G, mask=None):
    """mask: boolean (R,H,W,Cp), True where gy passes (the forward's y > 0), or None.  Returns (gx (R,H,W,Cp), ggamma (Cp,), gbeta (Cp,))."""
    gy, x, gamma, mean, rstd = (np.asarray(t, D) for t in (gy, x, gamma, mean, rstd))
    R, H, W, Cp = x.shape
    cpg = C // G
    dz = gy if mask is None else np.where(np.asarray(mask, bool), gy, 0.0)
    dzg, xg = _grouped(dz, C, G), _grouped(x, C, G)
    xh = (xg - mean[:, None, :, None]) * rstd[:, None, :, None]
    gt = dzg * gamma[:C].reshape(1, 1, G, cpg)
    a = gt.mean(axis=(1, 3), keepdims=True)
    b = (gt * xh).mean(axis=(1, 3), keepdims=True)
    gx = np.zeros((R, H, W, Cp), D)
    gx[..., :C] = (rstd[:, None, :, None] * (gt - a - xh * b)).reshape(R, H, W, C)
    ggamma, gbeta = np.zeros((Cp,), D), np.zeros((Cp,), D)
    ggamma[:C] = (dzg * xh).sum(axis=(0, 1)).reshape(C)
    gbeta[:C] = dzg.sum(axis=(0, 1)).reshape(C)
    return gx, ggamma, gbeta
