"""NumPy restatement of mrcnn_box_iou_loss_f32 (include/mrcnn_hip.h, csrc/box_loss.hip): loss, count and the
analytic gradient of the GIoU / DIoU / CIoU box regression losses on the decoded box.  Every operation runs in ``dtype``: float64 is the
reference the kernel is judged against, float32 the run that sets the gradient bound (tests/loss_judge.py).  Pinned against torch
float64 autograd by tests/test_box_iou_loss_cpu.py, which also holds the formulas written out in torch (``torch_loss``).

A helper of the tests, not a test and not part of the product."""
import numpy as np

GIOU, DIOU, CIOU = 1, 2, 3
KINDS = {'giou': GIOU, 'diou': DIOU, 'ciou': CIOU}
EPS = 1e-7
DSIZE_MAX = float(np.float32(np.log(1000.0 / 16.0)))     # the bound of the predicted dh, dw: the float32 the kernel compares against


def decode(v, rois, mean, std, dtype=np.float64, clamp=False):
    """(M,4) encoded deltas against (M,4) boxes (y1,x1,y2,x2) -> centre (cy, cx), size (h, w), the deltas d (M,4) before the clamp."""
    v, rois = np.asarray(v, dtype), np.asarray(rois, dtype)
    mean, std = np.asarray(mean, dtype), np.asarray(std, dtype)
    half = dtype(0.5)
    d = v * std + mean
    h, w = rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1]
    cy, cx = rois[:, 0] + half * h, rois[:, 1] + half * w
    dh, dw = (np.minimum(d[:, 2], dtype(DSIZE_MAX)), np.minimum(d[:, 3], dtype(DSIZE_MAX))) if clamp else (d[:, 2], d[:, 3])
    return d[:, 0] * h + cy, d[:, 1] * w + cx, np.exp(dh) * h, np.exp(dw) * w, d, h, w


def _axis(p1, p2, g1, g2, dtype):
    """Overlap i and enclosing side c of one axis with their derivatives by the prediction's centre (_c) and size (_s).  A tie of a
    min / max splits the derivative evenly (torch's rule); the clamp at 0 passes it where the overlap is positive."""
    raw = np.minimum(p2, g2) - np.maximum(p1, g1)
    i = np.maximum(raw, dtype(0))
    c = np.maximum(p2, g2) - np.minimum(p1, g1)
    share = lambda a, b: np.where(a > b, dtype(1), np.where(a == b, dtype(0.5), dtype(0)))       # of max(a, b) that belongs to a
    on = (raw > 0).astype(dtype)
    i1, i2 = on * share(p1, g1), on * share(g2, p2)
    c1, c2 = share(g1, p1), share(p2, g2)
    half = dtype(0.5)
    return i, c, i2 - i1, half * (i2 + i1), c2 - c1, half * (c2 + c1)


def rows(x, t, rois, kind, mean, std, dtype=np.float64):
    """Per-row loss L (M,) and d L / d x (M,4) of every row (labels not applied)."""
    kind = KINDS.get(kind, kind)
    if kind not in (GIOU, DIOU, CIOU):
        raise ValueError('kind %r' % (kind,))
    dt = dtype
    eps, half, one, two = dt(EPS), dt(0.5), dt(1), dt(2)
    std_ = np.asarray(std, dt)
    pcy, pcx, ph, pw, d, h, w = decode(x, rois, mean, std, dt, clamp=True)
    gcy, gcx, gh, gw, _, _, _ = decode(t, rois, mean, std, dt)
    py1, px1, py2, px2 = pcy - half * ph, pcx - half * pw, pcy + half * ph, pcx + half * pw
    gy1, gx1, gy2, gx2 = gcy - half * gh, gcx - half * gw, gcy + half * gh, gcx + half * gw
    ih, ch, ih_c, ih_s, ch_c, ch_s = _axis(py1, py2, gy1, gy2, dt)
    iw, cw, iw_c, iw_s, cw_c, cw_s = _axis(px1, px2, gx1, gx2, dt)
    inter = ih * iw
    uni = ((ph * pw + gh * gw) - inter) + eps
    iou = inter / uni
    L = one - iou
    zero = np.zeros_like(L)
    di = [ih_c * iw, ih_s * iw, ih * iw_c, ih * iw_s]            # derivatives by (pcy, ph, pcx, pw)
    da = [zero, pw, zero, ph]
    dL = [-((di[k] * (uni + inter) - inter * da[k]) / (uni * uni)) for k in range(4)]
    if kind == GIOU:
        c = ch * cw
        ce = c + eps
        L = L + (c - uni) / ce
        dc = [ch_c * cw, ch_s * cw, ch * cw_c, ch * cw_s]
        dL = [dL[k] + dc[k] * (uni + eps) / (ce * ce) - (da[k] - di[k]) / ce for k in range(4)]
    else:
        ry, rx = pcy - gcy, pcx - gcx
        rho2 = ry * ry + rx * rx
        dd = (ch * ch + cw * cw) + eps
        L = L + rho2 / dd
        q = rho2 / (dd * dd)
        dL[0] = dL[0] + (two * ry / dd - q * (two * ch * ch_c))
        dL[1] = dL[1] + (-q * (two * ch * ch_s))
        dL[2] = dL[2] + (two * rx / dd - q * (two * cw * cw_c))
        dL[3] = dL[3] + (-q * (two * cw * cw_s))
        if kind == CIOU:
            k4 = dt(4.0 / np.pi ** 2)
            hpe = ph + eps
            da_ = np.arctan(gw / (gh + eps)) - np.arctan(pw / hpe)
            v = k4 * (da_ * da_)
            alpha = v / (((one - iou) + v) + eps)                 # a constant in the gradient
            L = L + alpha * v
            den = hpe * hpe + pw * pw
            s = alpha * (two * k4) * da_
            dL[1] = dL[1] + s * (pw / den)
            dL[3] = dL[3] + (-s * (hpe / den))
    live_h, live_w = (d[:, 2] <= dt(DSIZE_MAX)).astype(dt), (d[:, 3] <= dt(DSIZE_MAX)).astype(dt)
    g = np.stack([dL[0] * h * std_[0], dL[2] * w * std_[1], live_h * (dL[1] * ph * std_[2]), live_w * (dL[3] * pw * std_[3])], 1)
    return L, g


def box_iou_loss(x, t, rois, label, kind, mean=(0, 0, 0, 0), std=(1, 1, 1, 1), weight=1.0, roi_period=None, dtype=np.float64):
    """-> (loss, count, gx (M,4)): loss = weight * sum of L over label > 0 / max(#(label >= 0), 1); gx = d loss / d x, zero rows for
    label <= 0.  rois (roi_period,4): row r is relative to rois[r % roi_period]."""
    x, t, rois, label = np.asarray(x), np.asarray(t), np.asarray(rois).reshape(-1, 4), np.asarray(label)
    M = x.shape[0]
    count = max(int((label >= 0).sum()), 1)
    g = np.zeros((M, 4), dtype)
    pos = np.nonzero(label > 0)[0]
    if not pos.size:
        return 0.0, count, g
    period = rois.shape[0] if roi_period is None else int(roi_period)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        L, gr = rows(x[pos], t[pos], rois[pos % period], kind, mean, std, dtype)
    scale = dtype(weight) / dtype(count)
    g[pos] = gr * scale
    return float(L.sum(dtype=dtype) * scale), count, g


# ---- the random inputs of the tests (tests/test_box_iou_loss_cpu.py checks them tie-free, tests/test_box_iou_loss_gpu.py runs the kernel on
# them) ----------------------------------------------------------------------------------------------------------------------------------
MEAN, STD = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)         # MaskRCNN.loc_normalize_mean / _std


def make_inputs(M=600, seed=0, tie_free=True):
    """M rows: RoIs and ground-truth boxes with corners up to 1200 px and sides 4..304 px, the gt near its RoI (IoU from 0 to high); the
    targets are the encoded gt, the predictions the targets plus noise; labels in -1..4.  tie_free: rows whose compared coordinates come
    closer than 1e-3 px are re-drawn (row_gaps)."""
    rs = np.random.RandomState(seed)

    def draw(n):
        side = rs.uniform(4.0, 304.0, (n, 2))
        tl = rs.uniform(0.0, 1200.0 - side)
        rois = np.concatenate([tl, tl + side], 1)
        gside = np.clip(side * np.exp(rs.uniform(-0.7, 0.7, (n, 2))), 4.0, 304.0)
        gc = tl + 0.5 * side + rs.uniform(-0.6, 0.6, (n, 2)) * side
        gtl = np.clip(gc - 0.5 * gside, 0.0, 1200.0 - gside)
        gt = np.concatenate([gtl, gtl + gside], 1)
        rois, gt = rois.astype(np.float32), gt.astype(np.float32)
        h, w = rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1]
        gh, gw = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
        loc = np.stack([(gt[:, 0] + 0.5 * gh - rois[:, 0] - 0.5 * h) / h, (gt[:, 1] + 0.5 * gw - rois[:, 1] - 0.5 * w) / w,
                        np.log(gh / h), np.log(gw / w)], 1)
        t = ((loc - np.asarray(MEAN)) / np.asarray(STD)).astype(np.float32)
        x = (t + rs.standard_normal((n, 4)) * 1.5).astype(np.float32)
        big = rs.rand(n, 2) < 0.03                       # a few predicted sizes above the clamp (dh = x * 0.2 > log(1000 / 16))
        x[:, 2:][big] = rs.uniform(21.0, 30.0, int(big.sum())).astype(np.float32)
        return x, t, rois
    x, t, rois = draw(M)
    if tie_free:
        for _ in range(20):
            bad = np.nonzero(row_gaps(x, t, rois) < 1e-3)[0]
            if not bad.size:
                break
            x[bad], t[bad], rois[bad] = draw(bad.size)
    label = rs.randint(-1, 5, M).astype(np.int32)
    return x, t, rois, label


def row_gaps(x, t, rois):
    """Per row, the smallest distance between two coordinates a min / max / clamp of the loss compares: P against G corner by corner,
    and the raw overlap of either axis against 0."""
    pcy, pcx, ph, pw, _, _, _ = decode(x, rois, MEAN, STD, clamp=True)
    gcy, gcx, gh, gw, _, _, _ = decode(t, rois, MEAN, STD)
    P = np.stack([pcy - ph / 2, pcx - pw / 2, pcy + ph / 2, pcx + pw / 2], 1)
    G = np.stack([gcy - gh / 2, gcx - gw / 2, gcy + gh / 2, gcx + gw / 2], 1)
    raw = np.stack([np.minimum(P[:, 2], G[:, 2]) - np.maximum(P[:, 0], G[:, 0]), np.minimum(P[:, 3], G[:, 3]) - np.maximum(P[:, 1], G[:, 1])], 1)
    return np.minimum(np.abs(P - G).min(1), np.abs(raw).min(1))
