"""NumPy restatements of the Mask Scoring R-CNN kernels (csrc/maskiou.hip) and of the MaskIoU head, in float64 (the
yardstick) and in float32 (operation for operation what the kernels compute; its own distance from float64 sets the tests' bars), and the
cases the CPU and GPU tests share.  The reference tree has no MaskIoU head, so nothing here is recorded from it.

A helper of the tests, not a test and not part of the product."""
import numpy as np

MASK_SIZE = 28
POOL = 14


# ---- the target ---------------------------------------------------------------------------------------------------------------------------
def mask_areas(masks, n_gt):
    """(N,G) int32: the nonzero bytes of every mask with g < n_gt[i]; 0 for the other slots whatever they hold."""
    N, G = masks.shape[:2]
    area = np.zeros((N, G), np.int32)
    for i in range(N):
        for g in range(min(max(int(n_gt[i]), 0), G)):
            area[i, g] = np.count_nonzero(masks[i, g])
    return area


def crop_rect(roi, H, W):
    """The rectangle k_mask_target crops: float32 corners truncated towards zero, clipped to the image."""
    y1, x1, y2, x2 = (int(np.float32(v)) for v in roi)
    return max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)


def target_counts(c, label_base=1):
    """counts (Rm,5) int64 = (full, crop, pred, gt28, ovr) of every mask row of case ``c``; zeros for padding rows and for rows whose
    channel is outside [0, n_channels): a label that selects a padding channel of mask_out has no class.  n_channels = c['n_fg']; every
    channel of mask_out for a case without that key."""
    masks, n_gt = c['masks'], c['n_gt']
    N, G, H, W = masks.shape
    rows, S = c['rows'], c['n_sample']
    area = mask_areas(masks, n_gt)
    out = np.zeros((N * rows, 5), np.int64)
    for r in range(N * rows):
        i, j = divmod(r, rows)
        srow = i * S + j
        ch = int(c['label'][r]) - label_base
        g = int(c['gt_assign'][srow])
        if not (j < c['n_pos'][i] and 0 <= ch < c.get('n_fg', c['mask_out'].shape[3]) and 0 <= g < min(G, int(n_gt[i]))):
            continue
        y0, y1, x0, x1 = crop_rect(c['sample_roi'][srow], H, W)
        crop = np.count_nonzero(masks[i, g, y0:y1, x0:x1]) if y1 > y0 and x1 > x0 else 0
        pred = c['mask_out'][r, :, :, ch] > 0
        gt = c['gt_roi_mask'][r] > 0
        out[r] = (area[i, g], crop, pred.sum(), gt.sum(), (pred & gt).sum())
    return out


def target_from_counts(counts, dtype=np.float64):
    """The float rule in ``dtype``: full_est = (gt28 * full) / crop; uni = (pred + full_est) - ovr; target = ovr / max(uni, 1); 0 where
    crop == 0 or full == 0.  In float32 every operation rounds once, in the kernel's order."""
    full, crop, pred, gt28, ovr = (counts[:, k].astype(dtype) for k in range(5))
    ok = (counts[:, 0] > 0) & (counts[:, 1] > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        full_est = (gt28 * full) / crop
        uni = (pred + full_est) - ovr
        t = ovr / np.maximum(uni, dtype(1))
    return np.where(ok, t, dtype(0)).astype(dtype)


def target(c, label_base=1, dtype=np.float64):
    return target_from_counts(target_counts(c, label_base), dtype)


# ---- the head's input ---------------------------------------------------------------------------------------------------------------------
def input_fwd(feat, mask_out, label, cin_p, label_base=1, n_channels=None):
    """(Rm,P,P,cin_p): channels [0,C) = feat, channel C = max(max(max(m[2y][2x], m[2y][2x+1]), m[2y+1][2x]), m[2y+1][2x+1]) of the row's
    channel (0 for a row without one: label - label_base outside [0, n_channels)), zeros behind.  n_channels None: every channel of
    mask_out is a class channel."""
    n_channels = mask_out.shape[3] if n_channels is None else n_channels
    Rm, P, _, C = feat.shape
    out = np.zeros((Rm, P, P, cin_p), feat.dtype)
    out[..., :C] = feat
    for r in range(Rm):
        ch = int(label[r]) - label_base
        if 0 <= ch < n_channels:
            m = mask_out[r, :, :, ch]
            out[r, :, :, C] = np.fmax(np.fmax(np.fmax(m[0::2, 0::2], m[0::2, 1::2]), m[1::2, 0::2]), m[1::2, 1::2])
    return out


def input_bwd(g_in, g_pool):
    """g_pool + g_in[..., :C]: one add per element in g_pool's dtype."""
    return g_pool + g_in[..., :g_pool.shape[3]].astype(g_pool.dtype)


# ---- the loss and the rescoring -----------------------------------------------------------------------------------------------------------
def l2(pred, tgt, label, weight=1.0, label_base=1, dtype=np.float64, n_channels=None):
    """(loss, count, gx): loss = weight * sum(0.5 d^2) / count over the rows with target > 0 and label - label_base in [0, n_channels)
    (None: every column of pred), d = pred[r, label - label_base] - target; gx = d * (weight * (1 / count)) in that column, zeros
    elsewhere; count = max(#rows, 1)."""
    pred, tgt = np.asarray(pred, dtype), np.asarray(tgt, dtype)
    Rm, ld = pred.shape
    ch = np.asarray(label, np.int64) - label_base
    on = (tgt > 0) & (ch >= 0) & (ch < (ld if n_channels is None else n_channels))
    rows = np.nonzero(on)[0]
    d = pred[rows, ch[rows]] - tgt[rows]
    count = dtype(max(len(rows), 1))
    loss = dtype(weight) * (dtype(0.5) * d * d).sum(dtype=dtype) / count
    gx = np.zeros((Rm, ld), dtype)
    gx[rows, ch[rows]] = d * (dtype(weight) * (dtype(1) / count))
    return dtype(loss), float(count), gx


def rescore(score, pred, label, n_channels=None):
    """score * min(max(pred[d, label[d]], 0), 1) in score's dtype; a label outside [0, n_channels) (None: the columns of pred) gives 0."""
    label = np.asarray(label, np.int64)
    ok = (label >= 0) & (label < (pred.shape[1] if n_channels is None else n_channels))
    iou = np.where(ok, pred[np.arange(pred.shape[0]), np.where(ok, label, 0)], pred.dtype.type(0))
    return score * np.fmin(np.fmax(iou, pred.dtype.type(0)), pred.dtype.type(1))


# ---- the head -----------------------------------------------------------------------------------------------------------------------------
HEAD_LAYERS = (('conv1', 3, 1, 1), ('conv2', 3, 1, 1), ('conv3', 3, 1, 1), ('conv4', 3, 2, 1))


def head_forward(params, x, dtype, prefix='head/maskiou/'):
    """The MaskIoU head on x (Rm,14,14,cin_p) with the store's padded parameters ``params`` (name -> array; W (cout_p,k,k,cin_p)): four
    3x3 convolutions (the last of stride 2) + ReLU, fc1 over the (h, w, c) flattening + ReLU, fc2 + ReLU, the output layer.  -> (Rm, out_p).
    torch on the CPU in ``dtype`` does the sums."""
    import torch
    import torch.nn.functional as F
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(td)
    h = t(x).permute(0, 3, 1, 2)
    for name, k, s, p in HEAD_LAYERS:
        w = t(params[prefix + name + '/W']).permute(0, 3, 1, 2)
        h = F.relu(F.conv2d(h, w, t(params[prefix + name + '/b']), stride=s, padding=p))
    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
    for name, relu in (('fc1', True), ('fc2', True), ('maskiou', False)):
        w = t(params[prefix + name + '/W'])
        h = h @ w.reshape(w.shape[0], -1).T + t(params[prefix + name + '/b'])
        if relu:
            h = F.relu(h)
    return h.numpy()


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def pad32(n):
    return (n + 31) // 32 * 32


def resize_nearest(crop, size=MASK_SIZE):
    """A (size,size) 0/1 int32 target of a crop (nearest sample; all zeros for an empty crop): a plausible gt_roi_mask for the cases - the
    kernel under test takes gt_roi_mask as an input, it does not make it."""
    h, w = crop.shape
    if h <= 0 or w <= 0:
        return np.zeros((size, size), np.int32)
    ys = np.minimum((np.arange(size) + 0.5) * h / size, h - 1).astype(np.int64)
    xs = np.minimum((np.arange(size) + 0.5) * w / size, w - 1).astype(np.int64)
    return (crop[ys][:, xs] != 0).astype(np.int32)


def _blob(rs, H, W):
    """A random ellipse inside the image; returns (mask u8, its bounding box y1, x1, y2, x2)."""
    h, w = rs.randint(max(H // 4, 2), max(H * 3 // 4, 3)), rs.randint(max(W // 4, 2), max(W * 3 // 4, 3))
    y1, x1 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
    yy, xx = np.mgrid[0:H, 0:W]
    m = (((yy - (y1 + (h - 1) / 2.0)) / (h / 2.0)) ** 2 + ((xx - (x1 + (w - 1) / 2.0)) / (w / 2.0)) ** 2 <= 1.0)
    return m.astype(np.uint8), (y1, x1, y1 + h, x1 + w)


def _logits(rs, gt, Cp, ch, flip=0.15):
    """(28,28,Cp) float32 logits: random everywhere, at channel ch of the sign of gt with a share ``flip`` of the positions flipped."""
    x = (rs.standard_normal((MASK_SIZE, MASK_SIZE, Cp)) * 2).astype(np.float32)
    if ch >= 0:
        sign = np.where(gt > 0, 1.0, -1.0) * np.where(rs.rand(MASK_SIZE, MASK_SIZE) < flip, -1.0, 1.0)
        x[:, :, ch] = (sign * (0.1 + np.abs(rs.standard_normal((MASK_SIZE, MASK_SIZE))))).astype(np.float32)
    return x


def random_case(seed, H, W, n_fg, N=2, G=4, n_gt=(3, 2), n_sample=12, rows=12, n_pos=(7, 5), junk=0):
    """Random live rows around the ground-truth boxes (fractional corners, some partly outside the image), padding rows behind n_pos."""
    rs = np.random.RandomState(seed)
    Cp = pad32(n_fg)
    masks = np.full((N, G, H, W), junk, np.uint8)
    boxes = np.zeros((N, G, 4), np.float64)
    gt_label = rs.randint(0, n_fg, (N, G))
    for i in range(N):
        for g in range(n_gt[i]):
            m, boxes[i, g] = _blob(rs, H, W)
            masks[i, g] = m * (255 if (i + g) % 3 == 0 else 1)          # nonzero is what counts, not one
    R, Rm = N * n_sample, N * rows
    sample_roi = np.zeros((R, 4), np.float32)
    gt_assign = np.full((R,), -1, np.int32)
    label = np.zeros((Rm,), np.int32)
    gt_roi_mask = np.full((Rm, MASK_SIZE, MASK_SIZE), -1, np.int32)
    mask_out = np.zeros((Rm, MASK_SIZE, MASK_SIZE, Cp), np.float32)
    for i in range(N):
        for j in range(n_sample):
            srow = i * n_sample + j
            if n_gt[i] > 0:
                g = rs.randint(0, n_gt[i])
                gt_assign[srow] = g
                b = boxes[i, g]
                hh, ww = b[2] - b[0], b[3] - b[1]
                jit = rs.uniform(-0.3, 0.3, 4) * (hh, ww, hh, ww)
                sample_roi[srow] = b + jit              # partly outside the image for boxes at its border
            if j >= rows:
                continue
            r = i * rows + j
            live = j < n_pos[i]
            if live:
                label[r] = gt_label[i, gt_assign[srow]] + 1
                y0, y1, x0, x1 = crop_rect(sample_roi[srow], H, W)
                gt_roi_mask[r] = resize_nearest(masks[i, gt_assign[srow], y0:max(y1, y0), x0:max(x1, x0)])
            mask_out[r] = _logits(rs, gt_roi_mask[r], Cp, label[r] - 1 if live else rs.randint(0, n_fg))
    return dict(masks=masks, n_gt=np.asarray(n_gt, np.int32), sample_roi=sample_roi, gt_assign=gt_assign, label=label,
                n_pos=np.asarray(n_pos, np.int32), n_sample=n_sample, rows=rows, mask_out=mask_out, gt_roi_mask=gt_roi_mask, n_fg=n_fg)


EDGE_ROWS = ('partly outside', 'no integer extent', 'the image', 'all-zero mask', 'crop 0, full > 0', 'all logits negative', 'exact one',
             'last channel', 'ordinary', 'behind n_pos', 'no assignment', 'background')


def edge_case(H, W, n_fg, rows=12, junk=255):
    """N = 2, G = 4, n_gt = (3, 0), n_sample = 12, n_pos = (9, 0): image 0's rows are EDGE_ROWS in order (rows 9 .. 11 are padding by one rule
    each), image 1 has no ground truth and no positive; the mask slots at and beyond n_gt hold ``junk``.  rows <= 12 keeps the first rows."""
    rs = np.random.RandomState(H * 131 + W + n_fg)
    N, G, S = 2, 4, 12
    Cp = pad32(n_fg)
    n_gt, n_pos = (3, 0), (min(9, rows), 0)
    masks = np.full((N, G, H, W), junk, np.uint8)
    masks[0, :3] = 0
    masks[0, 0, 5:20, 7:30] = 1                     # a 15 x 23 rectangle; rows below H, columns below W for 37 x 45 and 64 x 64
    masks[0, 0, 8:12, 10:14] = 0                    # with a hole
    masks[0, 1, H - 9:H, W - 11:W] = 255            # touching the bottom right corner
    # masks[0, 2] stays all zero
    R, Rm = N * S, N * rows
    roi = np.zeros((R, 4), np.float32)
    gt_assign = np.full((R,), -1, np.int32)
    lab = np.zeros((S,), np.int32)
    roi[0], gt_assign[0], lab[0] = (-6.5, -3.25, 14.75, 20.5), 0, 2
    roi[1], gt_assign[1], lab[1] = (5.2, 8.0, 5.9, 25.0), 0, 2
    roi[2], gt_assign[2], lab[2] = (0, 0, H, W), 0, 1
    roi[3], gt_assign[3], lab[3] = (2.0, 2.0, 30.0, 30.0), 2, 1
    roi[4], gt_assign[4], lab[4] = (22.5, 31.5, 35.0, 44.0), 0, 3
    roi[5], gt_assign[5], lab[5] = (4.0, 6.0, 22.0, 32.0), 0, 1
    roi[6], gt_assign[6], lab[6] = (3.9, 5.1, 21.5, 31.25), 0, 2
    roi[7], gt_assign[7], lab[7] = (H - 12.5, W - 14.0, H + 6.0, W + 9.5), 1, n_fg
    roi[8], gt_assign[8], lab[8] = (6.0, 9.0, 18.0, 27.0), 0, 1
    roi[9], gt_assign[9], lab[9] = (4.0, 6.0, 22.0, 32.0), 0, 2            # a live-looking row at n_pos
    roi[10], gt_assign[10], lab[10] = (4.0, 6.0, 22.0, 32.0), -1, 2
    roi[11], gt_assign[11], lab[11] = (4.0, 6.0, 22.0, 32.0), 0, 0
    roi[S:] = (1.0, 1.0, 20.0, 20.0)               # image 1: no positives; the assignments point at junk slots
    gt_assign[S:] = 1
    label = np.zeros((Rm,), np.int32)
    label[:rows] = lab[:rows]
    label[rows:] = 1
    gt_roi_mask = np.full((Rm, MASK_SIZE, MASK_SIZE), -1, np.int32)
    mask_out = np.zeros((Rm, MASK_SIZE, MASK_SIZE, Cp), np.float32)
    for r in range(Rm):
        i, j = divmod(r, rows)
        if i == 0 and j < n_pos[0]:
            y0, y1, x0, x1 = crop_rect(roi[j], H, W)
            gt_roi_mask[r] = resize_nearest(masks[0, gt_assign[j], y0:max(y1, y0), x0:max(x1, x0)])
        mask_out[r] = _logits(rs, gt_roi_mask[r], Cp, label[r] - 1)
    if rows > 5:
        mask_out[5] = -np.abs(mask_out[5]) - 0.5
    if rows > 6:
        mask_out[6, :, :, lab[6] - 1] = np.where(gt_roi_mask[6] > 0, 1.5, -0.25)
    return dict(masks=masks, n_gt=np.asarray(n_gt, np.int32), sample_roi=roi, gt_assign=gt_assign, label=label, n_pos=np.asarray(n_pos, np.int32),
                n_sample=S, rows=rows, mask_out=mask_out, gt_roi_mask=gt_roi_mask, n_fg=n_fg)


def target_cases():
    """[(name, case)]: the sizes of the issue - 37 x 45 (neither the mask's length nor its base a multiple of 16) and 64 x 64 -, 3 classes
    (Cp 32) and 80 (Cp 96), every row of the sampler block ('all') and its first rows ('positives'), random and edge rows."""
    out = []
    for H, W in ((37, 45), (64, 64)):
        for n_fg in (3, 80):
            out.append(('edge %dx%d c%d all' % (H, W, n_fg), edge_case(H, W, n_fg, rows=12)))
            out.append(('random %dx%d c%d all' % (H, W, n_fg), random_case(H + n_fg, H, W, n_fg)))
        out.append(('edge %dx%d c3 positives' % (H, W), edge_case(H, W, 3, rows=10)))
        out.append(('random %dx%d c80 positives' % (H, W), random_case(H + 7, H, W, 80, rows=8, n_pos=(8, 3))))
    out.append(('random 37x45 c3 no positives in image 1', random_case(99, 37, 45, 3, n_gt=(3, 0), n_pos=(6, 0), junk=255)))
    return out


def area_case(N, G, H, W, seed=0, junk=255):
    """Tiny masks for the area pass alone: random bytes (half of them zero, the others any value), n_gt random per image with the LAST
    image full (so mask N * G - 1 is read), image 0 at 0 and image 1 one below G, ``junk`` in the slots at and beyond n_gt; one live row per image on a
    1 x 1 logit map keeps the target pass cheap."""
    rs = np.random.RandomState(seed + N * G + H * W)
    masks = ((rs.rand(N, G, H, W) < 0.5) * rs.randint(1, 256, (N, G, H, W))).astype(np.uint8)
    masks[N - 1, G - 1].flat[0] = 3
    n_gt = rs.randint(1, G + 1, N).astype(np.int32)
    n_gt[N - 1] = G
    if N > 1:
        n_gt[0] = 0
    if N > 2:
        n_gt[1] = G - 1
    for i in range(N):
        masks[i, n_gt[i]:] = junk
    return dict(masks=masks, n_gt=n_gt, sample_roi=np.tile(np.array([0, 0, H, W], np.float32), (N, 1)),
                gt_assign=np.maximum(n_gt - 1, 0).astype(np.int32), label=np.ones((N,), np.int32), n_pos=np.ones((N,), np.int32), n_sample=1,
                rows=1, mask_out=np.ones((N, 1, 1, 32), np.float32), gt_roi_mask=np.ones((N, 1, 1), np.int32), n_fg=3)


CROP_WIDTHS, CROP_RESIDUES, CROP_HEIGHTS = (1, 15, 16, 17, 33), (0, 1, 15), (1, 40)


def crop_rects():
    """[(y0, x0, h, w)]: every width of CROP_WIDTHS at every start column residue mod 16 of CROP_RESIDUES, heights 1 and 40 in turn."""
    out = []
    for a, w in enumerate(CROP_WIDTHS):
        for b, res in enumerate(CROP_RESIDUES):
            out.append((2 + a, res + 16 * ((a + b) % 2), CROP_HEIGHTS[(a + b) % 2], w))
    return out


def crop_case(mask_size, H=48, W=51, n_fg=3, seed=0):
    """N = 2, G = 2, n_sample = 20, rows = 17 < n_sample: sampler row j crops crop_rects()[j] for j < 15 (fractional corners that truncate
    to it), row 15 is a live-looking row on a 30 x 40 crop whose label selects the first PADDING channel of mask_out (label = n_fg + 1: no class), row 16
    lies behind n_pos.  Every channel of mask_out, the padded ones included, is non-zero; gt_roi_mask is random 0 / 1."""
    rs = np.random.RandomState(seed + mask_size)
    N, G, S, rows = 2, 2, 20, 17
    Cp = pad32(n_fg)
    rects = crop_rects()
    masks = ((rs.rand(N, G, H, W) < 0.6) * rs.randint(1, 256, (N, G, H, W))).astype(np.uint8)
    roi = np.zeros((N * S, 4), np.float32)
    gt_assign = np.zeros((N * S,), np.int32)
    for i in range(N):
        for j in range(S):
            y0, x0, h, w = (4, 3, 30, 40) if j == 15 else rects[j % len(rects)]
            roi[i * S + j] = (y0 + 0.25, x0 + 0.5, y0 + h + 0.75, x0 + w + 0.25)
            gt_assign[i * S + j] = (i + j) % G
    label = rs.randint(1, n_fg + 1, N * rows).astype(np.int32)
    label[15::rows] = n_fg + 1
    mask_out = (rs.standard_normal((N * rows, mask_size, mask_size, Cp)) * 2).astype(np.float32)
    mask_out[mask_out == 0] = 1.0
    mask_out[15::rows, :, :, n_fg] = np.abs(mask_out[15::rows, :, :, n_fg])         # the padding channel would predict a full mask
    gt_roi_mask = (rs.rand(N * rows, mask_size, mask_size) < 0.6).astype(np.int32)
    gt_roi_mask[15::rows] = 1
    return dict(masks=masks, n_gt=np.array([G, G], np.int32), sample_roi=roi, gt_assign=gt_assign, label=label,
                n_pos=np.array([16, 16], np.int32), n_sample=S, rows=rows, mask_out=mask_out, gt_roi_mask=gt_roi_mask, n_fg=n_fg)
