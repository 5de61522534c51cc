"""Reference of the deformable convolution of csrc/deform.hip / nn.core.DeformConv in differentiable torch operations:
an explicit floor, four gathers and four weights per tap - no grid_sample - so that autograd gives the three gradients.  float64 by default;
``dtype=torch.float32`` evaluates the same expression in float32 on the CPU, whose error against float64 sets the bars of the sampling kernels
(tests/test_deform_gpu.py).  Tensors are NHWC like the library's:
  x (N,H,W,C); off (N,H,W,ld): (dy, dx) of tap k = 3 i + j in channels 2k, 2k + 1, modulated the logit of its mask in channel 18 + k, the rest
  of the row never read; w (Cout,3,3,C).
The sampling position of tap k of output pixel (y, x) is (y - 1 + i + dy, x - 1 + j + dx); a cell outside the map counts as zero, a position
at or beyond -1 or H (W) samples zero.
"""
import torch

TAPS = 9
OFFSET_CH = 18


def deform_cols(x, off, modulated, dtype=torch.float64):
    """The sampled columns (N,H,W,9,C)."""
    x, off = x.to(dtype), off.to(dtype)
    N, H, W, C = x.shape
    flat = x.reshape(N * H * W, C)
    n_ = torch.arange(N).view(N, 1, 1)
    ys = torch.arange(H).view(1, H, 1)
    xs = torch.arange(W).view(1, 1, W)
    cols = []
    for k in range(TAPS):
        i, j = divmod(k, 3)
        py = (ys - 1 + i).to(dtype) + off[..., 2 * k]
        px = (xs - 1 + j).to(dtype) + off[..., 2 * k + 1]
        inside = (py > -1) & (py < H) & (px > -1) & (px < W)
        py = torch.where(inside, py, torch.zeros_like(py))
        px = torch.where(inside, px, torch.zeros_like(px))
        fy, fx = torch.floor(py), torch.floor(px)
        ly, lx = py - fy, px - fx
        y0, x0 = fy.long(), fx.long()
        sample = torch.zeros((N, H, W, C), dtype=dtype)
        for a in (0, 1):
            for b in (0, 1):
                yy, xx = y0 + a, x0 + b
                ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                idx = (n_ * H + yy.clamp(0, H - 1)) * W + xx.clamp(0, W - 1)
                wgt = (ly if a else 1 - ly) * (lx if b else 1 - lx)
                sample = sample + (wgt * ok.to(dtype)).unsqueeze(-1) * flat[idx]
        if modulated:
            sample = sample * torch.sigmoid(off[..., OFFSET_CH + k]).unsqueeze(-1)
        cols.append(sample)
    return torch.stack(cols, 3)


def deform_conv(x, off, w, modulated, dtype=torch.float64):
    """y (N,H,W,Cout) of the layer: the columns times the filter, tap-major."""
    cols = deform_cols(x, off, modulated, dtype)
    Cout = w.shape[0]
    return torch.einsum('nhwkc,okc->nhwo', cols, w.to(dtype).reshape(Cout, TAPS, -1))


def cols_grads(x, off, g_cols, modulated, dtype=torch.float64):
    """(cols, gradient of x, gradient of the offset row) for the gradient g_cols (N,H,W,9,C) of the columns; the offset gradient is zero in
    the channels that are never read."""
    x = x.detach().to(dtype).requires_grad_(True)
    off = off.detach().to(dtype).requires_grad_(True)
    cols = deform_cols(x, off, modulated, dtype)
    gx, goff = torch.autograd.grad(cols, (x, off), g_cols.to(dtype).reshape(cols.shape))
    return cols.detach(), gx, goff


def conv_grads(x, off, w, gy, modulated, dtype=torch.float64):
    """(y, gx, goff, gw) of the whole layer for the gradient gy (N,H,W,Cout) of its output."""
    x = x.detach().to(dtype).requires_grad_(True)
    off = off.detach().to(dtype).requires_grad_(True)
    w = w.detach().to(dtype).requires_grad_(True)
    y = deform_conv(x, off, w, modulated, dtype)
    gx, goff, gw = torch.autograd.grad(y, (x, off, w), gy.to(dtype))
    return y.detach(), gx, goff, gw


def list_lengths(off, shape):
    """Entries per destination pixel (N,H,W) of the input gradient's inverted index: one for every (source pixel, tap, corner) whose cell
    lies inside the map, by the rule above in float32."""
    N, H, W, _ = shape
    off = off.float()
    n_ = torch.arange(N).view(N, 1, 1)
    ys = torch.arange(H).view(1, H, 1)
    xs = torch.arange(W).view(1, 1, W)
    counts = torch.zeros((N * H * W,), dtype=torch.int64)
    for k in range(TAPS):
        i, j = divmod(k, 3)
        py = (ys - 1 + i).float() + off[..., 2 * k]
        px = (xs - 1 + j).float() + off[..., 2 * k + 1]
        inside = (py > -1) & (py < H) & (px > -1) & (px < W)
        y0 = torch.floor(torch.where(inside, py, torch.zeros_like(py))).long()
        x0 = torch.floor(torch.where(inside, px, torch.zeros_like(px))).long()
        for a in (0, 1):
            for b in (0, 1):
                yy, xx = y0 + a, x0 + b
                ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                counts += torch.bincount(((n_ * H + yy.clamp(0, H - 1)) * W + xx.clamp(0, W - 1))[ok], minlength=N * H * W)
    return counts.view(N, H, W)
