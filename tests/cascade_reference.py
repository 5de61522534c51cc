"""The rules of the Cascade R-CNN stage-to-stage step (csrc/cascade.hip) restated in NumPy, in float64 or float32,
and the inference score of a cascade.  The float32 statement is the one of oracle/boxes.py (loc2bbox, bbox_iou, bbox2loc,
map_rois_to_fpn_levels; tests/test_cascade_cpu.py pins the two to each other), the float64 one what the kernels are judged against.

Row r of image i (R = N * S rows, image i owns rows [i * S, (i + 1) * S)):
  padding   prev_label[r] < 0: roi = 0, xy5 = (i,0,0,0,0), level 0, gt_loc = 0, label -1, assign -1.
  decode    d = box_out[r, loc0:loc0 + 4] * std_prev + mean; loc2bbox(rois[r], d); every corner clipped fmax(fmin(v, lim), 0) against the
            image's h / w (fmin / fmax drop a NaN, an infinite corner clips to the full extent: the box is always finite).  No clamp on dh / dw.
  level     map_rois_to_fpn_levels of the refined box (levels 0..4).
  xy5       (i, x1, y1, x2, y2).
  -- with ground truth --
  empty     y2 - y1 <= 0 or x2 - x1 <= 0: label -1, assign -1, gt_loc 0; the box and the level stay.
  no gt     G = min(n_gt[i], gt_cap) == 0: label 0, assign -1, gt_loc 0.
  match     bbox_iou against the image's first G boxes, NumPy's max / argmax (first maximum; a NaN wins, the first NaN stays); assign = argmax,
            label = gt_labels[argmax] + 1 where max >= iou_thresh (false for NaN), else 0.
  targets   label > 0: gt_loc = (bbox2loc(roi, gt[argmax]) - mean) / std_next; zeros elsewhere.

A helper of the tests, not a test and not part of the product."""
import numpy as np


def loc2bbox(src, loc, dt):
    src, loc = np.asarray(src, dt), np.asarray(loc, dt)
    h = src[:, 2] - src[:, 0]
    w = src[:, 3] - src[:, 1]
    cy = src[:, 0] + dt(0.5) * h
    cx = src[:, 1] + dt(0.5) * w
    with np.errstate(over='ignore', invalid='ignore'):
        ncy = loc[:, 0] * h + cy
        ncx = loc[:, 1] * w + cx
        nh = np.exp(loc[:, 2]) * h
        nw = np.exp(loc[:, 3]) * w
        return np.stack((ncy - dt(0.5) * nh, ncx - dt(0.5) * nw, ncy + dt(0.5) * nh, ncx + dt(0.5) * nw), axis=1).astype(dt)


def bbox2loc(src, dst, dt):
    src, dst = np.asarray(src, dt), np.asarray(dst, dt)
    h = src[:, 2] - src[:, 0]
    w = src[:, 3] - src[:, 1]
    cy = src[:, 0] + dt(0.5) * h
    cx = src[:, 1] + dt(0.5) * w
    bh = dst[:, 2] - dst[:, 0]
    bw = dst[:, 3] - dst[:, 1]
    bcy = dst[:, 0] + dt(0.5) * bh
    bcx = dst[:, 1] + dt(0.5) * bw
    eps = dt(np.finfo(np.float32).eps)
    h = np.maximum(h, eps)
    w = np.maximum(w, eps)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack(((bcy - cy) / h, (bcx - cx) / w, np.log(bh / h), np.log(bw / w)), axis=1).astype(dt)


def bbox_iou(a, b, dt):
    a, b = np.asarray(a, dt), np.asarray(b, dt)
    tl = np.maximum(a[:, None, :2], b[None, :, :2])
    br = np.minimum(a[:, None, 2:], b[None, :, 2:])
    area_i = np.prod(br - tl, axis=2) * (tl < br).all(axis=2)
    area_a = np.prod(a[:, 2:] - a[:, :2], axis=1)
    area_b = np.prod(b[:, 2:] - b[:, :2], axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (area_i / (area_a[:, None] + area_b - area_i)).astype(dt)


def level_argument(boxes, dt):
    """4 + log2(sqrt(area) / 224 + 1e-6): the level is its floor, clipped to 0..4.  float32: the logarithm is taken in double and rounded,
    as fpn_level of box_common.h does."""
    boxes = np.asarray(boxes, dt)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    v = np.sqrt(area) / dt(224) + dt(1e-6)
    return dt(4) + np.log2(v.astype(np.float64)).astype(dt)


def refine(rois, box_out, loc0, N, mean, std_prev, size, prev_label=None, gt_boxes=None, gt_labels=None, n_gt=None, iou_thresh=0.5,
           std_next=None, dtype=np.float64, details=False):
    """-> dict(roi, rois_xy5, levels[, gt_loc, label, gt_assign]); size: (N,2) array or one (h, w) pair.  details: also 'max_iou' and
    'second_iou' (the best and the second-best IoU of a matched row, NaN elsewhere) and 'level_arg' (NaN on padding rows)."""
    dt = np.dtype(dtype).type
    rois = np.asarray(rois, dt).reshape(-1, 4)
    R = rois.shape[0]
    S = R // N if N else 0
    box_out = np.asarray(box_out, dt).reshape(R, -1)
    mean, std_prev = np.asarray(mean, dt), np.asarray(std_prev, dt)
    size = np.asarray(size, dt)
    hw = size if size.ndim == 2 else np.tile(size[None], (max(N, 1), 1))
    train = gt_boxes is not None
    img = np.repeat(np.arange(N), S)
    live = np.ones(R, bool) if prev_label is None else np.asarray(prev_label).reshape(R) >= 0
    d = box_out[:, loc0:loc0 + 4] * std_prev + mean
    b = loc2bbox(rois, d, dt)
    lim_h, lim_w = hw[img, 0] if R else np.zeros(0, dt), hw[img, 1] if R else np.zeros(0, dt)
    b[:, 0] = np.fmax(np.fmin(b[:, 0], lim_h), dt(0))
    b[:, 2] = np.fmax(np.fmin(b[:, 2], lim_h), dt(0))
    b[:, 1] = np.fmax(np.fmin(b[:, 1], lim_w), dt(0))
    b[:, 3] = np.fmax(np.fmin(b[:, 3], lim_w), dt(0))
    b[~live] = 0
    with np.errstate(divide='ignore'):
        larg = level_argument(b, dt)
    lev = np.clip(np.floor(larg), 0, 4).astype(np.int32)
    lev[~live] = 0
    xy5 = np.concatenate([img[:, None].astype(dt), b[:, [1, 0, 3, 2]]], axis=1)
    out = dict(roi=b, rois_xy5=xy5, levels=lev)
    if details:
        out['level_arg'] = np.where(live, larg, np.nan)
    if not train:
        return out
    gt_boxes = np.asarray(gt_boxes, dt)
    gt_labels = np.asarray(gt_labels)
    gt_cap = gt_boxes.shape[1]
    std_next = np.asarray(std_next, dt)
    loc = np.zeros((R, 4), dt)
    label = np.full(R, -1, np.int32)
    assign = np.full(R, -1, np.int32)
    max_iou = np.full(R, np.nan)
    second = np.full(R, np.nan)
    for i in range(N):
        G = max(min(int(n_gt[i]), gt_cap), 0)
        rows = np.arange(i * S, (i + 1) * S)
        bb = b[rows]
        ok = live[rows] & ~((bb[:, 2] - bb[:, 0] <= 0) | (bb[:, 3] - bb[:, 1] <= 0))
        rows = rows[ok]
        if not rows.size:
            continue
        label[rows] = 0
        if G == 0:
            continue
        iou = bbox_iou(b[rows], gt_boxes[i, :G], dt)
        arg = iou.argmax(axis=1)                 # NumPy: the first maximum; a NaN wins and the first NaN stays
        mx = iou.max(axis=1)
        assign[rows] = arg
        max_iou[rows] = mx
        if G > 1:
            second[rows] = np.sort(np.where(np.isnan(iou), -np.inf, iou), axis=1)[:, -2]
        with np.errstate(invalid='ignore'):
            fg = mx >= dt(iou_thresh)
        lab = np.where(fg, gt_labels[i, arg].astype(np.int64) + 1, 0)
        label[rows] = lab
        pos = rows[lab > 0]
        if pos.size:
            loc[pos] = (bbox2loc(b[pos], gt_boxes[i, assign[pos]], dt) - mean) / std_next
    out.update(gt_loc=loc, label=label, gt_assign=assign)
    if details:
        out.update(max_iou=max_iou, second_iou=second)
    return out


def softmax_rows(o, n_class, dt):
    o = np.asarray(o, dt)[:, :n_class]
    e = np.exp(o - o.max(axis=1, keepdims=True))
    s = np.zeros(o.shape[0], dt)
    for c in range(n_class):                     # the class-order sum of detect_decode_row
        s = s + e[:, c]
    return e / s[:, None]


def prob_mean(box_outs, n_class, dtype=np.float64):
    """((p1 + p2) + p3) / K of the stages' softmax over the first n_class columns."""
    dt = np.dtype(dtype).type
    p = softmax_rows(box_outs[0], n_class, dt)
    for b in box_outs[1:]:
        p = p + softmax_rows(b, n_class, dt)
    return p / dt(len(box_outs))


# ---- the fixed random cases of tests/test_cascade_cpu.py and tests/test_cascade_gpu.py ----------------------------------------------
LOC0 = 84                 # the head's box_out layout: 81 scores, padding, the class-agnostic loc at column 84 of 88
LD = 88
MEAN = (0., 0., 0., 0.)
STDS = ((0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1), (0.033, 0.033, 0.067, 0.067))
GEOMETRIES = (((2, 8, 4), (3, 0)), ((2, 64, 5), (5, 4)), ((1, 300, 3), (3,)))
SEEDS = {(2, 8, 4): 11, (2, 64, 5): 12, (1, 300, 3): 13}


def random_case(geom, n_gt, seed):
    """Ground truth in a 128 x 160 (second image 112 x 144) frame, proposals jittered around it so that every IoU band is populated, deltas
    of the size a trained stage gives, padding rows at the end of each image block.  All float32 values."""
    N, S, G = geom
    rs = np.random.RandomState(seed)
    hw = np.array([[128., 160.], [112., 144.]], np.float32)[:N]
    gt = np.zeros((N, G, 4), np.float32)
    labels = np.full((N, G), -1, np.int32)
    rois = np.zeros((N, S, 4), np.float32)
    prev = np.zeros((N, S), np.int32)
    for i in range(N):
        h, w = hw[i]
        cy, cx = rs.uniform(20, h - 20, G), rs.uniform(20, w - 20, G)
        bh, bw = rs.uniform(16, 70, G), rs.uniform(16, 90, G)
        gt[i] = np.stack([np.maximum(cy - bh / 2, 0), np.maximum(cx - bw / 2, 0), np.minimum(cy + bh / 2, h), np.minimum(cx + bw / 2, w)], 1)
        gt[i, 0] = (2, 2, h - 2, w - 2)      # one object fills the frame: every refined box overlaps some ground truth, so no row's best two
        labels[i, :n_gt[i]] = rs.randint(0, 80, n_gt[i])        # IoUs are both 0 (a tie that the first-maximum rule alone would decide)
        src = gt[i, rs.randint(0, max(n_gt[i], 1), S)] if n_gt[i] else gt[i, rs.randint(0, G, S)]
        sh, sw = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
        jit = rs.uniform(-0.3, 0.3, (S, 4)) * np.stack([sh, sw, sh, sw], 1)
        r = src + jit
        r = np.stack([np.minimum(r[:, 0], r[:, 2] - 2), np.minimum(r[:, 1], r[:, 3] - 2), r[:, 2], r[:, 3]], 1)
        far = rs.uniform(0, 1, S) < 0.2                     # a fifth of the rows are boxes anywhere in the image
        y1, x1 = rs.uniform(0, h - 12, S), rs.uniform(0, w - 12, S)
        anyb = np.stack([y1, x1, y1 + rs.uniform(8, 60, S), x1 + rs.uniform(8, 60, S)], 1)
        rois[i] = np.where(far[:, None], anyb, r)
        n_pad = max(1, S // 8)
        prev[i, S - n_pad:] = -1
        rois[i, S - n_pad:] = 0
        prev[i, :S - n_pad] = rs.randint(0, 3, S - n_pad)
    box_out = rs.standard_normal((N * S, LD)).astype(np.float32)
    box_out[:, LOC0:LOC0 + 4] = (rs.standard_normal((N * S, 4)) * [1.0, 1.0, 0.6, 0.6]).astype(np.float32)
    return dict(N=N, S=S, G=G, rois=rois.reshape(-1, 4), box_out=box_out, prev_label=prev.reshape(-1), gt_boxes=gt, gt_labels=labels,
                n_gt=np.asarray(n_gt, np.int32), hw=hw, pair=(float(hw[0, 0]), float(hw[0, 1])))


def random_cases():
    """(name, case, iou_thresh, std_prev, std_next, size) for every geometry x threshold x size form."""
    out = []
    for geom, n_gt in GEOMETRIES:
        case = random_case(geom, n_gt, SEEDS[geom])
        for thr, sp, sn in ((0.6, STDS[0], STDS[1]), (0.7, STDS[1], STDS[2])):
            for form in ('per_image', 'pair'):
                out.append(('%dx%dx%d-%.1f-%s' % (geom + (thr, form)), case, thr, sp, sn, case['hw'] if form == 'per_image' else case['pair']))
    return out


def run_case(case, thr, sp, sn, size, dtype, details=False):
    return refine(case['rois'], case['box_out'], LOC0, case['N'], MEAN, sp, size, case['prev_label'], case['gt_boxes'], case['gt_labels'],
                  case['n_gt'], thr, sn, dtype=dtype, details=details)


# ---- the hand-built edge cases: exact arithmetic (zero deltas: expf(0) = 1; unit std) ------------------------------------------------
EDGE_THRESH = 0.75
EDGE_STD = (1., 1., 1., 1.)


def edge_case():
    """Three 100 x 100 images of four rows each; 'expect' holds the hand-derived integer outputs and boxes.
      image 0: two identical ground-truth boxes (10,10,50,50) with labels 3 and 7
        row 0  (10,10,50,40): IoU 1200 / 1600 = 0.75 exactly = the threshold -> foreground; the tie of the two boxes takes the first
        row 1  (80,80,90,90) with dy = dx = +5: pushed to (130,130,140,140), clips to (100,100,100,100): empty -> label -1, box finite
        row 2  (20,20,40,40) with dh = dw = +88: expf(88) * 20 overflows -> the full extent (0,0,100,100), IoU 0.16 -> background
        row 3  (12,12,48,52): IoU 1368 / 1672 -> foreground with non-zero targets
      image 1: no ground truth -> rows 4 and 6 are background with assign -1, rows 5 and 7 are padding (their inputs are garbage)
      image 2: one zero-area ground-truth box (60,60,60,80) -> row 8 (55,55,70,85) has IoU 0: background, zero targets, no NaN;
        rows 9-11 padding."""
    N, S, G = 3, 4, 2
    rois = np.zeros((N * S, 4), np.float32)
    box_out = np.zeros((N * S, LD), np.float32)
    prev = np.zeros(N * S, np.int32)
    rois[0] = (10, 10, 50, 40)
    rois[1] = (80, 80, 90, 90)
    box_out[1, LOC0:LOC0 + 2] = 5
    rois[2] = (20, 20, 40, 40)
    box_out[2, LOC0 + 2:LOC0 + 4] = 88
    rois[3] = (12, 12, 48, 52)
    rois[4] = (5, 5, 30, 30)
    rois[6] = (40, 20, 90, 70)
    rois[8] = (55, 55, 70, 85)
    for r in (5, 7, 9, 10, 11):
        prev[r] = -1
        rois[r] = (3, 4, 50, 60)
        box_out[r] = 1e30
    gt = np.zeros((N, G, 4), np.float32)
    gt[0, 0] = gt[0, 1] = (10, 10, 50, 50)
    gt[2, 0] = (60, 60, 60, 80)
    labels = np.full((N, G), -1, np.int32)
    labels[0] = (3, 7)
    labels[2, 0] = 5
    n_gt = np.array([2, 0, 1], np.int32)
    box = rois.copy()
    box[1] = (100, 100, 100, 100)
    box[2] = (0, 0, 100, 100)
    box[[5, 7, 9, 10, 11]] = 0
    expect = dict(label=np.array([4, -1, 0, 4, 0, -1, 0, -1, 0, -1, -1, -1], np.int32),
                  gt_assign=np.array([0, -1, 0, 0, -1, -1, -1, -1, 0, -1, -1, -1], np.int32),
                  levels=np.array([1, 0, 2, 1, 0, 0, 1, 0, 0, 0, 0, 0], np.int32), roi=box)
    return dict(N=N, S=S, G=G, rois=rois, box_out=box_out, prev_label=prev, gt_boxes=gt, gt_labels=labels, n_gt=n_gt, pair=(100., 100.),
                hw=np.full((N, 2), 100, np.float32), expect=expect)
