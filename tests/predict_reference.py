"""NumPy float64 restatement of the single-view inference post-processing (csrc/predict.hip, arithmetic in csrc/detect_common.h), written
from the rules the kernels replace (oracle/predict.py states the same rules in the kernels' own precision):

  * decode: un-scale, de-normalise, loc2bbox, clip, softmax - every value float64 from the float32 inputs on.  The parameters (scale,
    mean, std, size) are taken as the float32 values the entry point receives.  Also returns the unclipped centre and size per axis,
    the scale the box judge measures an error against (tests/predict_judge.py);
  * paste: v64 = 255 * bilinear(sigmoid(logit)), or 255 * bilinear(prob), per pixel of the box window.  The interpolation coefficients and
    tap indices are cv2's float32 ones (oracle.predict.cv2_resize_linear_f32: they are part of the rule, not rounding); the sigmoid
    and the three lerps are float64.  paste_f32 is the same walk in float32, operation for operation the oracle's, kept as a value
    (the oracle truncates it to uint8 at once);
  * suppression is index work: keep_lists is oracle.predict.suppress, split into the per-class rows the kernels write.

Pinned by tests/test_predict_cases_cpu.py.  A helper of the tests, not a test and not part of the product."""
import numpy as np

from oracle import predict as op

D = np.float64
F = np.float32


def _f32(v):
    return np.asarray(v, F).astype(D)


def decode(rois, box_out, n_class, loc0, scale, mean, std, size):
    """rois (R,4), box_out (R,ld) float32 -> dict(bbox (R,4) clipped, prob (R,n_class), centre (R,2) = (ncy, ncx) and size (R,2) =
    (nh, nw) before the clip, raw (R,4) = the box before the clip), all float64."""
    roi = np.asarray(rois, F).astype(D) / _f32(scale)
    o = np.asarray(box_out, F).astype(D)
    loc = o[:, loc0:loc0 + 4] * _f32(std) + _f32(mean)
    h, w = roi[:, 2] - roi[:, 0], roi[:, 3] - roi[:, 1]
    cy, cx = roi[:, 0] + 0.5 * h, roi[:, 1] + 0.5 * w
    ncy, ncx = loc[:, 0] * h + cy, loc[:, 1] * w + cx
    nh, nw = np.exp(loc[:, 2]) * h, np.exp(loc[:, 3]) * w
    raw = np.stack([ncy - 0.5 * nh, ncx - 0.5 * nw, ncy + 0.5 * nh, ncx + 0.5 * nw], 1)
    bbox = raw.copy()
    bbox[:, 0::2] = np.clip(bbox[:, 0::2], 0.0, float(F(size[0])))
    bbox[:, 1::2] = np.clip(bbox[:, 1::2], 0.0, float(F(size[1])))
    x = o[:, :n_class]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return dict(bbox=bbox, prob=e / e.sum(axis=1, keepdims=True), centre=np.stack([ncy, ncx], 1), size=np.stack([nh, nw], 1), raw=raw)


def sigmoid(x):
    x = np.asarray(x, D)
    e = np.exp(-np.abs(x))                      # never overflows
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_f32(x):
    """The oracle's float32 sigmoid (oracle.predict.paste_masks)."""
    with np.errstate(over='ignore'):
        return (F(1) / (F(1) + np.exp(-np.asarray(x, F)))).astype(F)


def cv2_linear_coef(ssize, dsize):
    """cv2.resize INTER_LINEAR along one axis, ssize -> dsize samples: (i0, i1 int64, f float32) with dst[d] = src[i0[d]] * (1 - f[d]) +
    src[i1[d]] * f[d].  Half-pixel centres in double, rounded to float32, edge clamp - oracle.predict.cv2_resize_linear_f32's ``coef``."""
    scale = 1.0 / (float(dsize) / float(ssize))
    v = ((np.arange(dsize, dtype=D) + 0.5) * scale - 0.5).astype(F)
    s = np.floor(v).astype(np.int64)
    f = (v - s.astype(F)).astype(F)
    lo, hi = s < 0, s >= ssize - 1
    f[lo | hi] = F(0)
    s[lo] = 0
    s[hi] = ssize - 1
    return s, np.minimum(s + 1, ssize - 1), f


def window(box, size):
    """(int(y1), int(x1), mh, mw, hh, ww) of one float32 box: the paste origin, the resize target int(y2 - y1) x int(x2 - x1) (the
    difference taken in float32, then truncated) and its part inside the image."""
    b = np.asarray(box, F)
    mh, mw = int(b[2] - b[0]), int(b[3] - b[1])
    s, t = int(b[0]), int(b[1])
    return s, t, mh, mw, max(min(mh, size[0] - s), 0), max(min(mw, size[1] - t), 0)


def _resize(m, mh, mw, dtype):
    y0, y1, fy = cv2_linear_coef(m.shape[0], mh)
    x0, x1, fx = cv2_linear_coef(m.shape[1], mw)
    fy, fx, one = fy.astype(dtype), fx.astype(dtype), dtype(1)
    rows = (m[:, x0] * (one - fx)[None, :] + m[:, x1] * fx[None, :]).astype(dtype)         # horizontal, then vertical
    return (rows[y0] * (one - fy)[:, None] + rows[y1] * fy[:, None]).astype(dtype)


def paste(maps, bbox, size, from_logits):
    """maps (D,S,S) float32 - the selected channel's logits, or probabilities - and bbox (D,4) float32 -> per detection a dict(win = (s, t,
    mh, mw, hh, ww), v = (hh, ww) float64 255 * bilinear(...) over the part of the window inside the image; None for an empty window)."""
    out = []
    for m, b in zip(maps, bbox):
        win = window(b, size)
        s, t, mh, mw, hh, ww = win
        v = None
        if mh > 0 and mw > 0 and hh > 0 and ww > 0:
            m64 = sigmoid(m) if from_logits else np.asarray(m, F).astype(D)
            v = (_resize(m64, mh, mw, D) * 255.0)[:hh, :ww]
        out.append(dict(win=win, v=v))
    return out


def paste_f32(maps, bbox, size, from_logits):
    """The same in float32, operation for operation oracle.predict.paste_masks: v = resize(m) * 255 before the truncation to uint8."""
    out = []
    for m, b in zip(maps, bbox):
        win = window(b, size)
        s, t, mh, mw, hh, ww = win
        v = None
        if mh > 0 and mw > 0 and hh > 0 and ww > 0:
            m32 = sigmoid_f32(m) if from_logits else np.asarray(m, F)
            v = (op.cv2_resize_linear_f32(m32, (mw, mh)) * F(255)).astype(F)[:hh, :ww]
        out.append(dict(win=win, v=v))
    return out


def masks_from(pasted, size):
    """(D,H,W) bool of paste / paste_f32 values: v >= 128 (= uint8(v) > 127 for 0 <= v <= 255) inside the window, 0 outside."""
    out = np.zeros((len(pasted),) + tuple(size), bool)
    for i, p in enumerate(pasted):
        if p['v'] is not None:
            s, t, _, _, hh, ww = p['win']
            out[i, s:s + hh, t:t + ww] = p['v'] >= 128
    return out


def keep_lists(cls_bbox, prob, n_class, l_begin, l_end, score_thresh, nms_thresh):
    """oracle.predict.suppress on the float32 boxes and scores the device gets, as the rows the kernels write: {l: RoI indices in
    selection order} for l in [l_begin, l_end).  suppress runs the classes 1 .. n_class - 1, without the last one under predict_mask."""
    if l_begin != 1 or l_end not in (n_class - 1, n_class):
        raise ValueError('the oracle runs the classes [1, n_class - 1) or [1, n_class)')
    idx, lab = op.suppress(np.asarray(cls_bbox, F), np.asarray(prob, F), n_class, nms_thresh, score_thresh, predict_mask=l_end == n_class - 1)
    return {l: idx[lab == l - 1] for l in range(l_begin, l_end)}


def keypoint_decode(heat, bbox, K):
    """NumPy restatement of mrcnn_keypoint_decode_f32: heat (D,S,S,Cp), bbox (D,4) float32 -> idx (D,K) int, y, x, logit (D,K) float32
    (the first maximum of channel k, the top-left corner of its cell mapped into the box in float32), prob (D,K) float64."""
    Dn, S = heat.shape[0], heat.shape[1]
    h = heat[..., :K].transpose(0, 3, 1, 2).reshape(Dn, K, S * S)
    idx = h.argmax(-1)
    logit = h.max(-1)
    y1, x1, y2, x2 = (bbox[:, j:j + 1] for j in range(4))
    y = (idx // S).astype(F) * ((y2 - y1) / F(S)) + y1
    x = (idx % S).astype(F) * ((x2 - x1) / F(S)) + x1
    prob = 1.0 / np.exp(h.astype(D) - logit[..., None].astype(D)).sum(-1)
    return idx, y, x, logit, prob
