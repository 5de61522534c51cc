"""NumPy restatement of the PointRend rules (csrc/pointrend.hip, csrc/point_common.h), the yardstick of
tests/test_pointrend_cpu.py and tests/test_pointrend_gpu.py.  Every function takes ``dt``: np.float64 is the reference proper; np.float32
rounds every operation as the kernels do - one rounding per product and per sum, the four tap products added in tap order, no contraction -
so the kernels must equal it bit for bit.  A helper of the tests, not a test and not part of the product."""
import numpy as np

U24 = 2.0 ** -24


def pad32(n):
    return (n + 31) // 32 * 32


def key_unit(keys, dt=np.float32):
    """(key >> 8) * 2^-24 of uint32 keys (held in an int32 or uint32 array): exact in float32."""
    k = np.asarray(keys).astype(np.int64) & 0xffffffff
    return ((k >> 8).astype(np.float64) * U24).astype(dt)


def taps(px, py, W, H, dt):
    """x0, y0 (int64; clamped to [-2, size] like the kernel's conversion) and the four weights of the taps (y0,x0), (y0,x0+1), (y0+1,x0),
    (y0+1,x0+1)."""
    px, py = np.asarray(px, dt), np.asarray(py, dt)
    half, one = dt(0.5), dt(1)
    fx, fy = px - half, py - half
    x0, y0 = np.floor(fx), np.floor(fy)
    lx, ly = fx - x0, fy - y0
    w = [(one - ly) * (one - lx), (one - ly) * lx, ly * (one - lx), ly * lx]
    return np.clip(x0, -2, W).astype(np.int64), np.clip(y0, -2, H).astype(np.int64), w


def point_sample(amap, px, py, dt, clamp=False):
    """amap (H,W) or (H,W,C); px, py arrays of one shape -> the rule's value at every point (shape + (C,)).  clamp: the tap indices are
    clamped to the map (the subdivision's upsample) instead of contributing zero outside it."""
    amap = np.asarray(amap)
    H, W = amap.shape[:2]
    x0, y0, w = taps(px, py, W, H, dt)
    s = np.zeros(x0.shape + amap.shape[2:], dt)
    for k in range(4):
        x, y = x0 + (k & 1), y0 + (k >> 1)
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        v = amap[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(dt)
        wk = w[k].reshape(w[k].shape + (1,) * (amap.ndim - 2))
        term = s + wk * v
        if clamp:
            s = term
        else:
            s = np.where(inside.reshape(wk.shape), term, s)
    return s


def abs_bits(val):
    """The ranking key of the kernels: the uint32 bits of |value| in float32.  Ascending in |value| for finite input; +-0 -> 0, denormals
    above it, +-inf above every finite value, a NaN (its sign cleared) above inf."""
    return np.abs(np.asarray(val).astype(np.float32)).view(np.uint32)


def rank(val):
    """Indices of ``val`` in ascending abs_bits order, ties to the lower index (a stable sort)."""
    return np.argsort(abs_bits(np.asarray(val).reshape(-1)), kind='stable')


def frame(rois_xy5, coords, dt):
    """X = x1 + u (x2 - x1), Y = y1 + v (y2 - y1) for coords (rows,P,2) of boxes (rows,5) (idx,x1,y1,x2,y2)."""
    r = np.asarray(rois_xy5).astype(dt)
    c = np.asarray(coords).astype(dt)
    X = r[:, None, 1] + c[..., 0] * (r[:, None, 3] - r[:, None, 1])
    Y = r[:, None, 2] + c[..., 1] * (r[:, None, 4] - r[:, None, 2])
    return X, Y


def features_fwd(coords, rois_xy5, fmap, scale, coarse, n_fg, cin_p, dt):
    """The head's input (rows,P,cin_p): fmap (N,H,W,C) at (X scale, Y scale), coarse (rows,S0,S0,Cp)[..., :n_fg] at (u S0, v S0), zeros."""
    rows, P = coords.shape[:2]
    C, S0 = fmap.shape[3], coarse.shape[1]
    X, Y = frame(rois_xy5, coords, dt)
    sc = dt(np.float32(scale))
    out = np.zeros((rows, P, cin_p), dt)
    c = np.asarray(coords).astype(dt)
    for r in range(rows):
        idx = int(rois_xy5[r, 0])
        if 0 <= idx < fmap.shape[0]:
            out[r, :, :C] = point_sample(fmap[idx], X[r] * sc, Y[r] * sc, dt)
        out[r, :, C:C + n_fg] = point_sample(coarse[r][..., :n_fg], c[r, :, 0] * dt(S0), c[r, :, 1] * dt(S0), dt)
    return out


def features_bwd(g_in, coords, rois_xy5, scale, g_map, dt, unit_weights=False):
    """g_map (N,H,W,C) plus the fine part of g_in (rows,P,ld) in the kernel's order: the value the map holds is the first addend, then
    w * g of every tap in ascending (row, point) order (a point's four taps land on four different cells).  unit_weights: every tap inside
    the map counts with weight 1 (the tests' error bounds: how many taps, and how much |g|, land on a cell)."""
    out = np.array(g_map, dt)
    N, H, W, C = out.shape
    rows, P = coords.shape[:2]
    X, Y = frame(rois_xy5, coords, dt)
    sc = dt(np.float32(scale))
    x0, y0, w = taps(X * sc, Y * sc, W, H, dt)
    g = np.asarray(g_in).reshape(rows, P, -1)[..., :C].astype(dt)
    for r in range(rows):
        idx = int(rois_xy5[r, 0])
        if not 0 <= idx < N:
            continue
        for p in range(P):
            for k in range(4):
                x, y = x0[r, p] + (k & 1), y0[r, p] + (k >> 1)
                if 0 <= x < W and 0 <= y < H:
                    out[idx, y, x] = out[idx, y, x] + (dt(1) if unit_weights else w[k][r, p]) * g[r, p]
    return out


def candidate_values(keys, coarse, label, n_fg, n_cand, label_base=1, dt=np.float32):
    """(rows,n_cand): the coarse logit of the row's channel sampled at every candidate; zeros for a row without a channel."""
    keys = np.asarray(keys)
    rows, S0 = coarse.shape[0], coarse.shape[1]
    unit = key_unit(keys, dt)
    val = np.zeros((rows, n_cand), dt)
    with np.errstate(invalid='ignore'):
        for r in range(rows):
            ch = int(label[r]) - label_base
            if 0 <= ch < n_fg:
                val[r] = point_sample(coarse[r][..., ch], unit[r, 0:2 * n_cand:2] * dt(S0), unit[r, 1:2 * n_cand:2] * dt(S0), dt)
    return val


def train_coords(keys, coarse, label, n_fg, P, n_cand, n_imp, label_base=1, dt=np.float32):
    """coords (rows,P,2) and the ranked candidate indices (rows,n_imp).  The ranking is the kernel's: ascending uint32 bits of |coarse
    logit at the candidate| in float32 (abs_bits), ties to the lower candidate index (a stable sort); a row without a channel has
    uncertainty 0 everywhere."""
    keys = np.asarray(keys)
    rows, S0 = coarse.shape[0], coarse.shape[1]
    unit = key_unit(keys, dt)
    coords = np.zeros((rows, P, 2), dt)
    picked = np.zeros((rows, n_imp), np.int64)
    for r in range(rows):
        ch = int(label[r]) - label_base
        u, v = unit[r, 0:2 * n_cand:2], unit[r, 1:2 * n_cand:2]
        val = np.zeros((n_cand,), dt)
        if 0 <= ch < n_fg:
            with np.errstate(invalid='ignore'):
                val = point_sample(coarse[r][..., ch], u * dt(S0), v * dt(S0), dt)
        order = rank(val)[:n_imp]
        picked[r] = order
        coords[r, :n_imp, 0], coords[r, :n_imp, 1] = u[order], v[order]
        rest = unit[r, 2 * n_cand:2 * n_cand + 2 * (P - n_imp)]
        coords[r, n_imp:, 0], coords[r, n_imp:, 1] = rest[0::2], rest[1::2]
    return coords, picked


def live_rows(n_gt, gt_assign, label, n_pos, n_sample, rows, G):
    """The live rule of the MaskIoU target: slot below n_pos[i], label > 0, assignment in [0, min(G, n_gt[i]))."""
    Rm = len(label)
    live = np.zeros((Rm,), bool)
    for r in range(Rm):
        i, j = divmod(r, rows)
        g = int(gt_assign[i * n_sample + j])
        live[r] = j < n_pos[i] and label[r] > 0 and 0 <= g < min(G, int(n_gt[i]))
    return live


def target(masks, n_gt, rois_xy5, gt_assign, label, n_pos, n_sample, rows, coords, dt):
    """Soft targets (Rm,P): the assigned mask read as 1.0 / 0.0 at (X, Y); -1 in the rows that are not live."""
    N, G, H, W = masks.shape
    live = live_rows(n_gt, gt_assign, label, n_pos, n_sample, rows, G)
    X, Y = frame(rois_xy5, coords, dt)
    out = np.full(coords.shape[:2], -1, dt)
    for r in np.nonzero(live)[0]:
        i, j = divmod(int(r), rows)
        out[r] = point_sample((masks[i, gt_assign[i * n_sample + j]] != 0).astype(dt), X[r], Y[r], dt)
    return out


def bce(pred, tgt, label, n_fg, weight, label_base=1, dt=np.float64):
    """(loss, count, gradient) of the point loss: pred (rows,P,ld), tgt (rows,P) with negative = skipped, label (rows,)."""
    pred = np.asarray(pred)
    rows, P = tgt.shape
    pred = pred.reshape(rows, P, -1)
    gx = np.zeros(pred.shape, dt)
    total, count = dt(0), 0
    ch = np.asarray(label).astype(np.int64) - label_base
    terms = []
    for r in range(rows):
        if not 0 <= ch[r] < n_fg:
            continue
        ok = tgt[r] >= 0
        x, t = pred[r, ok, ch[r]].astype(dt), tgt[r, ok].astype(dt)
        terms.append(np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x))))
        count += int(ok.sum())
    cnt = max(count, 1)
    if terms:
        total = np.concatenate(terms).sum(dtype=dt)
    for r in range(rows):
        if not 0 <= ch[r] < n_fg:
            continue
        ok = tgt[r] >= 0
        x, t = pred[r, ok, ch[r]].astype(dt), tgt[r, ok].astype(dt)
        gx[r, ok, ch[r]] = (dt(1) / (dt(1) + np.exp(-x)) - t) * (dt(weight) * (dt(1) / dt(cnt)))
    return dt(weight) * total / dt(cnt), cnt, gx


def upsample2x(grid, dt):
    """(S,S) -> (2S,2S): the value at cell (y, x) is the grid at the centre ((x + 0.5) / 2, (y + 0.5) / 2), taps clamped to the grid."""
    S = grid.shape[0]
    c = (np.arange(2 * S).astype(dt) + dt(0.5)) * dt(0.5)
    return point_sample(grid, c[None, :].repeat(2 * S, 0), c[:, None].repeat(2 * S, 1), dt, clamp=True)


def subdivide(grid, n_points, dt=np.float32):
    """grid (D,S,S) -> (up (D,2S,2S), index (D,n_sel) ascending flat cells, coords (D,n_sel,2)): the n_sel = min(n_points, 4 S^2) cells of
    smallest |up| by abs_bits, ties to the lower flat index."""
    D, S = grid.shape[:2]
    n_sel = min(n_points, 4 * S * S)
    with np.errstate(invalid='ignore'):
        up = np.stack([upsample2x(g, dt) for g in grid]) if D else np.zeros((0, 2 * S, 2 * S), dt)
    index = np.zeros((D, n_sel), np.int32)
    for d in range(D):
        index[d] = np.sort(rank(up[d])[:n_sel])
    x, y = index % (2 * S), index // (2 * S)
    coords = np.stack([(x.astype(dt) + dt(0.5)) / dt(2 * S), (y.astype(dt) + dt(0.5)) / dt(2 * S)], -1)
    return up, index, coords


def concat_fwd(h, x0, c0, n_coarse, cin_p):
    """[h (n,Ch) | x0 (n,ld0)[:, c0 : c0 + n_coarse] | zeros] -> (n,cin_p): a copy, no arithmetic."""
    n, Ch = h.shape
    out = np.zeros((n, cin_p), h.dtype)
    out[:, :Ch] = h
    out[:, Ch:Ch + n_coarse] = x0[:, c0:c0 + n_coarse]
    return out


def concat_bwd(g_in, Ch):
    """g_in (n,cin_p)[:, :Ch]: the hidden part of the gradient; the coarse part is dropped."""
    return np.ascontiguousarray(g_in[:, :Ch])


# ---- the point head ---------------------------------------------------------------------------------------------------------------------
LAYERS = ('fc1', 'fc2', 'fc3', 'predictor')


def head_forward(params, x0, C, n_fg, dt, prefix='head/point/'):
    """params: name -> array (padded shapes (cout_p,1,1,cin_p) / (cout_p,)); x0 (n, cin_p).  Returns (pred (n, out_p), tape)."""
    x0 = np.asarray(x0).astype(dt)
    coarse = x0[:, C:C + n_fg]
    x, tape, h = x0, [], None
    for i, name in enumerate(LAYERS):
        W = params[prefix + name + '/W'].astype(dt)
        W = W.reshape(W.shape[0], W.shape[-1])
        b = params[prefix + name + '/b'].astype(dt)
        if i:
            x = np.zeros((x0.shape[0], W.shape[1]), dt)
            x[:, :h.shape[1]] = h
            x[:, h.shape[1]:h.shape[1] + n_fg] = coarse
        y = x @ W.T + b
        if name != 'predictor':
            y = np.maximum(y, 0)
        tape.append((x, y, W))
        h = y
    return h, tape


def head_backward(tape, g_pred, C, dt):
    """-> (parameter gradients name -> array in the padded shapes, the input gradient (n, cin_p))."""
    g = np.asarray(g_pred).astype(dt).reshape(tape[-1][1].shape)
    grads = {}
    for i in range(len(LAYERS) - 1, -1, -1):
        x, y, W = tape[i]
        if LAYERS[i] != 'predictor':
            g = g * (y > 0)
        grads[LAYERS[i] + '/W'] = (g.T @ x).reshape(W.shape[0], 1, 1, W.shape[1])
        grads[LAYERS[i] + '/b'] = g.sum(0)
        gx = g @ W
        if i:
            g = gx[:, :tape[i - 1][1].shape[1]]
    return grads, gx


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def feature_case(H, W, C, P, n_fg=3, S0=6, seed=0):
    """Five rows on two images: a box partly outside the map, one thinner than a cell, an ordinary one, and two overlapping boxes on
    different images.  The map has stride 4 (scale 0.25)."""
    rs = np.random.RandomState(seed + H * W + C + P)
    fh, fw = 4.0 * H, 4.0 * W
    rois = np.array([[0, -9.5, -6.25, 0.45 * fw, 0.5 * fh],             # partly outside
                     [1, 0.3 * fw, 0.2 * fh, 0.3 * fw + 1.5, 0.9 * fh],  # thinner than a cell
                     [0, 0.1 * fw, 0.3 * fh, 0.8 * fw, 0.95 * fh],
                     [0, 0.5 * fw, 0.4 * fh, fw + 7.0, fh + 3.0],        # overlaps the next, on the other image, and leaves the map
                     [1, 0.5 * fw, 0.4 * fh, 0.9 * fw, 0.8 * fh]], np.float32)
    coords = rs.rand(5, P, 2).astype(np.float32)
    coords[0, 0] = (0.0, 0.0)
    Cp = pad32(n_fg)
    return dict(rois=rois, coords=coords, fmap=rs.standard_normal((2, H, W, C)).astype(np.float32),
                coarse=(rs.standard_normal((5, S0, S0, Cp)) * 3).astype(np.float32), n_fg=n_fg, cin_p=pad32(C + n_fg),
                g_in=rs.standard_normal((5, P, pad32(C + n_fg))).astype(np.float32),
                g_map=rs.standard_normal((2, H, W, C)).astype(np.float32))


def general_feature_case(N, H, W, C, P, rows, n_fg, S0, cin_p, seed, rois=None, ld=None, coords=None):
    """Any sizes: ``rows`` random boxes around the stride-4 map's frame (some partly outside), image indices cycling over [0, N), or the
    boxes given (rows,5).  coarse (rows,S0,S0,Cp) is non-zero in EVERY channel, the padded ones included; g_in (rows,P,ld) is non-zero
    behind the fine channels too (ld defaults to cin_p)."""
    rs = np.random.RandomState(seed)
    fh, fw = 4.0 * H, 4.0 * W
    if rois is None:
        rois = np.zeros((rows, 5), np.float32)
        rois[:, 0] = np.arange(rows) % N
        x1, y1 = rs.uniform(-0.1, 0.7, rows) * fw, rs.uniform(-0.1, 0.7, rows) * fh
        rois[:, 1], rois[:, 2] = x1, y1
        rois[:, 3], rois[:, 4] = x1 + rs.uniform(0.05, 0.5, rows) * fw, y1 + rs.uniform(0.05, 0.5, rows) * fh
    rois = np.asarray(rois, np.float32)
    assert rois.shape == (rows, 5)
    if coords is None:
        coords = rs.rand(rows, P, 2).astype(np.float32)
    Cp = pad32(n_fg)
    ld = cin_p if ld is None else ld
    coarse = (rs.standard_normal((rows, S0, S0, Cp)) * 3).astype(np.float32)
    coarse[coarse == 0] = 1.0
    return dict(rois=rois, coords=np.asarray(coords, np.float32), fmap=rs.standard_normal((N, H, W, C)).astype(np.float32), coarse=coarse,
                n_fg=n_fg, cin_p=cin_p, g_in=rs.standard_normal((rows, P, ld)).astype(np.float32),
                g_map=rs.standard_normal((N, H, W, C)).astype(np.float32))


def target_case(H=37, W=45, P=9, seed=1):
    """2 images x 6 rows of an n_sample = 8 sampler, G = 3 slots: live rows, a point on the image border, an unused mask slot filled with
    junk, and a non-live row of every kind (behind n_pos, background, padding label, assignment at n_gt, negative assignment)."""
    rs = np.random.RandomState(seed)
    N, G, n_sample, rows = 2, 3, 8, 6
    masks = (rs.rand(N, G, H, W) < 0.5).astype(np.uint8) * rs.randint(1, 256, (N, G, H, W)).astype(np.uint8)
    n_gt = np.array([2, 3], np.int32)
    masks[0, 2] = 255                                   # the unused slot of image 0: junk
    n_pos = np.array([5, 4], np.int32)
    gt_assign = np.array([0, 1, 1, 2, -1, 0, 0, 0,      # image 0: row 3 assigned at n_gt, row 4 negative, row 5 behind n_pos
                          2, 0, 1, 2, 0, 0, 0, 0], np.int32)
    label = np.array([1, 2, 0, 1, 1, 1,                 # image 0: row 2 background
                      3, -1, 1, 2, 1, 1], np.int32)     # image 1: row 1 padding label, rows 4, 5 behind n_pos
    rois = np.zeros((N * rows, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), rows)
    x1, y1 = rs.rand(N * rows) * W * 0.5, rs.rand(N * rows) * H * 0.5
    rois[:, 1], rois[:, 2] = x1, y1
    rois[:, 3], rois[:, 4] = x1 + 4 + rs.rand(N * rows) * W * 0.6, y1 + 4 + rs.rand(N * rows) * H * 0.6
    rois[0, 1:] = (0.0, 0.0, W, H)                      # the whole image: the point (0, 0) lies on its border
    coords = rs.rand(N * rows, P, 2).astype(np.float32)
    coords[0, 0] = (0.0, 0.0)
    coords[0, 1] = (1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24)
    return dict(masks=masks, n_gt=n_gt, rois=rois, gt_assign=gt_assign, label=label, n_pos=n_pos, n_sample=n_sample, rows=rows, coords=coords)
