"""NumPy float32 restatement of the rules of Soft-NMS, box voting and the detection cap (include/mrcnn_hip.h mrcnn_class_soft_nms_f32 /
mrcnn_box_vote_f32, MaskRCNN._suppress), written from the rules: every operation on float32 values rounds once,
as the kernels' do (no contraction, correctly rounded division).  A helper of the tests (tests/test_boxpost_cpu.py,
tests/test_boxpost_gpu.py), not a test and not part of the product."""
import numpy as np

F = np.float32
METHODS = ('hard', 'linear', 'gaussian')


def box_iou(b, c):
    """IoU of box b (4,) against the boxes c (n,4): ai / ((area_b + area_c) - ai), float32 (n,).  Two zero-area boxes give NaN."""
    b, c = np.asarray(b, F), np.asarray(c, F).reshape(-1, 4)
    with np.errstate(invalid='ignore', divide='ignore'):
        area_b = (b[2] - b[0]) * (b[3] - b[1])
        top, left = np.fmax(b[0], c[:, 0]), np.fmax(b[1], c[:, 1])
        bottom, right = np.fmin(b[2], c[:, 2]), np.fmin(b[3], c[:, 3])
        ai = np.fmax(bottom - top, F(0)) * np.fmax(right - left, F(0))
        return (ai / ((area_b + (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])) - ai)).astype(F)


def weight(method, iou, nms_thresh, sigma):
    """The factor on a remaining candidate's score at this IoU (float32 array); a NaN IoU gives 1."""
    iou = np.asarray(iou, F)
    one = np.ones_like(iou)
    with np.errstate(invalid='ignore'):
        if method == 'hard':
            return np.where(iou >= F(nms_thresh), F(0), one).astype(F)
        if method == 'linear':
            return np.where(iou >= F(nms_thresh), F(1) - iou, one).astype(F)
        if method == 'gaussian':
            return np.where(iou > F(0), np.exp((-(iou * iou)) / F(sigma)).astype(F), one).astype(F)
    raise ValueError(method)


def soft_nms_class(box, p, score_thresh, method, nms_thresh, sigma):
    """Soft-NMS of one class: box (R,4), p (R,) = prob[:, l].  Returns (rows, scores, k, gap): the selected rows in selection order, their
    decayed float32 scores, k = the largest number of non-unit decays any candidate received, gap = the smallest relative gap this run met
    between the top two scores of an arg-max (ties excluded: the index decides them) and between a decayed score and score_thresh
    (inf when it met none)."""
    box, p, thresh = np.asarray(box, F), np.asarray(p, F), F(score_thresh)
    with np.errstate(invalid='ignore'):
        cand = np.nonzero(p > thresh)[0]
    s = p[cand].copy()
    alive = np.ones(len(cand), bool)
    decays = np.zeros(len(cand), np.int64)
    rows, scores, gap = [], [], np.inf
    while alive.any():
        live = np.nonzero(alive)[0]
        top = s[live].max()
        ties = live[s[live] == top]
        m = ties[-1]                                # score descending, then index descending (cand ascends)
        if len(ties) == 1 and len(live) > 1:
            second = s[live[live != m]].max()
            gap = min(gap, float((np.float64(top) - np.float64(second)) / abs(np.float64(top))))
        rows.append(int(cand[m]))
        scores.append(s[m])
        alive[m] = False
        rest = np.nonzero(alive)[0]
        if not len(rest):
            break
        w = weight(method, box_iou(box[cand[m]], box[cand[rest]]), nms_thresh, sigma)
        new = (s[rest] * w).astype(F)
        hit = w != F(1)
        decays[rest] += hit
        if hit.any():
            d = np.abs(new[hit].astype(np.float64) - np.float64(thresh)) / max(abs(float(thresh)), np.finfo(F).tiny)
            gap = min(gap, float(d.min()))
        s[rest] = new
        with np.errstate(invalid='ignore'):
            alive[rest] = new > thresh
    return np.asarray(rows, np.int64), np.asarray(scores, F), int(decays.max()) if len(decays) else 0, gap


def class_soft_nms(cls_bbox, prob, l_begin, l_end, score_thresh, method, nms_thresh, sigma):
    """All classes of [l_begin, l_end): ({l: rows}, {l: scores}, k, gap) with k / gap over the classes."""
    rows, scores, k, gap = {}, {}, 0, np.inf
    for l in range(l_begin, l_end):
        rows[l], scores[l], kl, gl = soft_nms_class(cls_bbox, np.asarray(prob)[:, l], score_thresh, method, nms_thresh, sigma)
        k, gap = max(k, kl), min(gap, gl)
    return rows, scores, k, gap


def vote_class(box, p, score_thresh, vote_thresh, rows):
    """Box voting of one class for the kept rows: (boxes (K,4) float64 = the weighted means in float64 of the float32 inputs, sizes (K,)
    = |V_k|).  An empty vote set leaves the kept box."""
    box, p = np.asarray(box, F), np.asarray(p, F)
    with np.errstate(invalid='ignore'):
        cand = np.nonzero(p > F(score_thresh))[0]
    out, sizes = np.zeros((len(rows), 4), np.float64), np.zeros(len(rows), np.int64)
    for j, k in enumerate(rows):
        with np.errstate(invalid='ignore'):
            v = cand[box_iou(box[k], box[cand]) >= F(vote_thresh)]
        sizes[j] = len(v)
        if len(v):
            wgt = p[v].astype(np.float64)
            out[j] = (wgt[:, None] * box[v].astype(np.float64)).sum(0) / wgt.sum()
        else:
            out[j] = box[k]
    return out, sizes


def cap(score, max_detections):
    """Indices kept by the detection cap, ascending: the max_detections highest scores, ties to the earlier row."""
    score = np.asarray(score, F)
    if max_detections is None or len(score) <= max_detections:
        return np.arange(len(score))
    order = np.argsort(-score.astype(np.float64), kind='stable')[:max_detections]
    return np.sort(order)


def suppress(cls_bbox, prob, l_end, score_thresh, nms_thresh, method='hard', sigma=0.5, vote_thresh=None, max_detections=None):
    """MaskRCNN._suppress with the three features: classes 1 .. l_end-1 concatenated in selection order, then the cap.  Returns (rows,
    label int32, score float32, bbox float64 (the voted boxes, or the kept rows' own), n_l = candidates of every detection's class)."""
    cls_bbox, prob = np.asarray(cls_bbox, F), np.asarray(prob, F)
    rows, lab, score, bbox, n_l = [], [], [], [], []
    for l in range(1, l_end):
        r, s, _, _ = soft_nms_class(cls_bbox, prob[:, l], score_thresh, method, nms_thresh, sigma)
        rows.append(r)
        lab.append(np.full(len(r), l - 1, np.int32))
        score.append(s)
        bbox.append(vote_class(cls_bbox, prob[:, l], score_thresh, vote_thresh, r)[0] if vote_thresh is not None
                    else cls_bbox[r].astype(np.float64))
        n_l.append(np.full(len(r), int((prob[:, l] > F(score_thresh)).sum()), np.int64))
    rows, lab, score = np.concatenate(rows), np.concatenate(lab), np.concatenate(score).astype(F)
    bbox, n_l = np.concatenate(bbox).reshape(-1, 4), np.concatenate(n_l)
    keep = cap(score, max_detections)
    return rows[keep], lab[keep], score[keep], bbox[keep], n_l[keep]
