"""Edge cases of the single-view inference post-processing kernels (k_detect_decode, k_class_nms, k_mask_paste of csrc/predict.hip,
k_mask_paste_prob of csrc/tta.hip, the keypoint decode of csrc/keypoints.hip; arithmetic in csrc/detect_common.h) as pure-NumPy builders.
Every builder returns the inputs of one device call, the float64 restatement's outputs (tests/predict_reference.py), the float32
oracle's (oracle/predict.py) and the tolerance the oracle's own error gives (tests/predict_judge.py).  No GPU import:
tests/test_predict_cases_cpu.py asserts from NumPy alone that each case sits on the edge it is named for and that the oracle passes the
judges; tests/test_predict_gpu.py and tests/test_keypoint_predict_gpu.py compare the kernels with the same dictionaries.  Every shape is the
smallest that still reaches its branch; each case is built once per process and must not be modified.

Decode (13 cases): R in {1, 255, 256, 257} (the 256-thread block edge) x (n_class, ld, loc0) in {(81, 96, 88), (2, 8, 4), (21, 25, 21)} -
the keypoint model's two classes, and ld == loc0 + 4 with a loc0 that is no multiple of 4 - with the scales 1.25, 0.7, 1/3 and the means 0
and (0.1, -0.2, 0.05, -0.05) spread over them; and ``planted``: a box beyond each of the four sides, two wholly outside, a zero-height and
a zero-width RoI, dh = dw = +-4, a softmax row with one logit 100 above the rest, a row of equal logits, at the rows 0.., 255 and 256.

Suppression: n_class = 5, l_begin = 1, l_end in {4, 5}.  ``grid``: R in {1, 63, 64, 65, 255, 256, 257, 511, 512} (+ 513 for the workspace
kernel) - the nw = ceil(n / 64) word count at 64 / 65, the 256-thread strides at 256 / 257, CN_CAP = 512 - scores k / 64 (ties), 10 % of
the boxes exact duplicates, score_thresh = 0.25: class 1 and 4 have every score above it (n == R), class 2 has 5 % of them exactly on it
and 5 % below, class 3 has no candidate.  ``identical``: one box R times (cnt == 1, the survivor the highest index of the top score).
``disjoint``: cnt == n, the order score descending then index descending.  ``threshold`` (nms_thresh = 0.5): (0,0,10,10) against
(0,0,10,5) has IoU exactly 0.5 in float32 and is suppressed by >=, the same pair with the 5 one ulp lower is kept and one ulp higher is
suppressed; two zero-area boxes on one spot (0 / 0: both kept) and one inside a normal box (IoU 0).

Paste (for mrcnn_mask_paste_f32 and, from float32 probabilities, mrcnn_mask_paste_prob_f32): S in {14, 28, 56}, Cm in {96, 4, 1} with the
labels 0 and Cm - 1, the images 1 x 1, 1 x 40, 40 x 1, 97 x 131 and 513 x 512 (262,656 pixels > 1024 workgroups x 256: the grid-stride loop's
second trip, a box in the last rows), D = 0; boxes of 1 x 1, 5 x 9 (downscale), S x S (identity), 2S x (2S + 1), 7 x 300, the whole image,
y1 = 3.7 / y2 = 10.2 (int(y2 - y1) = 6, not 7), zero height, width 0.9, one in the last row and column.  Logits of standard deviation 2.

Keypoint decode: S in {7, 14, 28, 56} x (K, Cp) in {(4, 4), (5, 8), (17, 32), (33, 64), (256, 256)} - lanes per cell P in {1, 2, 8, 16, 64} -
x D in {1, 3} (K = 256 at S = 56: D = 1), and D = 300 at S = 14, K = 17 (more detections than the grid's 2048-workgroup target divided by
the largest split count; the split count there is 3, the floor of 196 cells / (32 cells a step x 2)).  The split counts reached are
1, 3, 6, 12, 24, 49, 98, 392 (keypoint_geometry restates the entry point's rule); planted ties, an all-equal channel, padding channels at 1e4.

Measured (the float32 oracle against float64 by the judges' own ratios on the CPU, tests/test_predict_cases_cpu.py -s prints them; the
kernels on an MI355X, tests/test_predict_gpu.py -s):
  decode boxes   oracle 1.7e-8 .. 1.9e-7 over the 13 cases, so every case's rtol is the floor 16 eps32 = 1.9e-6; kernels 1.7e-8 .. 1.9e-7
  decode probs   oracle 6.8e-8 (2 classes) .. 1.3e-6 (81 classes), rtol 1.9e-6 .. 5.1e-6; kernels 1.8e-7 .. 1.5e-6
  paste          oracle worst |v32 - v64| 4.1e-5 from logits, 3.3e-5 from probabilities; band 1.2e-4 (the floor, the small images) ..
                 1.6e-4; pixels of the reference within the band: 0 of 76,886 in-box pixels over the 8 cases, for either entry point"""
import functools
import re

import numpy as np

from oracle import predict as op
from tests import predict_judge as pj
from tests import predict_reference as ref

F = np.float32
IMG = (480, 500)                                    # decode: the original image the boxes are clipped to
STD = (0.1, 0.1, 0.2, 0.2)
MEAN0, MEAN1 = (0., 0., 0., 0.), (0.1, -0.2, 0.05, -0.05)
DECODE_R = [1, 255, 256, 257]
DECODE_LAYOUTS = [(81, 96, 88), (2, 8, 4), (21, 25, 21)]
DECODE_SCALES = [1.25, 0.7, 1.0 / 3.0]
CN_CAP = 512                                        # detect_common.h: most RoIs of the all-in-LDS class NMS


# ======================================================================================================================
# A. decode
# ======================================================================================================================
def _decode_rows(rs, R, n_class, ld, loc0, scale):
    c = np.stack([rs.uniform(20, IMG[0] - 20, R), rs.uniform(20, IMG[1] - 20, R)], 1)
    hw = np.exp(rs.uniform(np.log(8), np.log(300), (R, 2)))
    rois = (np.concatenate([c - hw / 2, c + hw / 2], 1) * scale).astype(F)
    box = (rs.standard_normal((R, ld)) * 7).astype(F)                      # the columns that are neither score nor loc must not matter
    box[:, :n_class] = rs.standard_normal((R, n_class)) * 3
    box[:, loc0:loc0 + 4] = rs.standard_normal((R, 4)) * 0.5
    return rois, box


def _decode_finish(name, rois, box, n_class, loc0, scale, mean, planted=None):
    want = ref.decode(rois, box, n_class, loc0, scale, mean, STD, IMG)
    ob_, op_ = op.decode(rois, box[:, loc0:loc0 + 4], box[:, :n_class], scale, IMG, n_class, mean=mean, std=STD)
    return dict(name=name, rois=rois, box_out=box, n_class=n_class, loc0=loc0, scale=scale, mean=mean, std=STD, size=IMG, want=want,
                oracle_bbox=ob_, oracle_prob=op_, box_rtol=pj.box_rtol(ob_, want), prob_rtol=pj.rtol_from(op_, want['prob']),
                planted=planted or {})


DECODE_NAMES = ['R%d-c%d' % (R, lay[0]) for R in DECODE_R for lay in DECODE_LAYOUTS] + ['planted']


@functools.lru_cache(maxsize=None)
def decode_case(name):
    if name == 'planted':
        return _decode_planted()
    i, j = [(i, j) for i, R in enumerate(DECODE_R) for j, lay in enumerate(DECODE_LAYOUTS) if name == 'R%d-c%d' % (R, lay[0])][0]
    R, (n_class, ld, loc0) = DECODE_R[i], DECODE_LAYOUTS[j]
    scale, mean = DECODE_SCALES[(i + j) % 3], (MEAN1 if (i + j) % 2 else MEAN0)
    rois, box = _decode_rows(np.random.RandomState(100 + 10 * i + j), R, n_class, ld, loc0, scale)
    return _decode_finish(name, rois, box, n_class, loc0, scale, mean)


def _decode_planted():
    R, (n_class, ld, loc0), scale, mean = 257, DECODE_LAYOUTS[0], 1.25, MEAN1
    rs = np.random.RandomState(7)
    rois, box = _decode_rows(rs, R, n_class, ld, loc0, scale)
    rows = {}

    def plant(key, row, roi=None, loc=None, logits=None):
        rows[key] = row
        if roi is not None:
            rois[row] = np.asarray(roi, np.float64) * scale
            box[row, loc0:loc0 + 4] = 0 if loc is None else loc
        if logits is not None:
            box[row, :n_class] = logits
    raw = lambda d, k: (d - mean[k]) / STD[k]                                # the box_out value that de-normalises to d
    plant('top', 0, (-40, 100, 30, 200))
    plant('left', 1, (100, -40, 200, 30))
    plant('bottom', 2, (450, 100, 520, 200))
    plant('right', 3, (100, 470, 200, 540))
    plant('outside_high', 4, (600, 600, 700, 700))
    plant('outside_low', 5, (-200, -200, -100, -100))
    plant('zero_height', 6, (100, 100, 100, 200))
    plant('zero_width', 255, (100, 100, 200, 100))
    plant('exp_plus4', 7, (200, 200, 210, 210), (0, 0, raw(4.0, 2), raw(4.0, 3)))
    plant('exp_minus4', 256, (200, 200, 210, 210), (0, 0, raw(-4.0, 2), raw(-4.0, 3)))
    sat = (rs.standard_normal(n_class) * 0.5).astype(F)
    sat[17] = sat.max() + F(100)
    plant('saturated', 8, logits=sat)
    plant('equal', 9, logits=np.full(n_class, 1.5, F))
    return _decode_finish('planted', rois, box, n_class, loc0, scale, mean, planted=rows)


# ======================================================================================================================
# B. suppression
# ======================================================================================================================
NMS_N_CLASS, NMS_SCORE_THRESH = 5, 0.25
NMS_GRID_R = [1, 63, 64, 65, 255, 256, 257, 511, 512]
NMS_NAMES = (['grid-R%d-e%d' % (R, e) for R in NMS_GRID_R for e in (4, 5)] +
             ['%s-e%d' % (s, e) for s in ('identical', 'disjoint', 'threshold') for e in (4, 5)])
NMS_OVER_CAP = 'grid-R513-e5'                       # the workspace kernel only


def iou_f32(b, c):
    """box_common.h's nms_iou, the IoU inside nms_suppresses, in float32 NumPy (oracle.boxes.nms's expression)."""
    b, c = np.asarray(b, F), np.asarray(c, F)
    top, left, bottom, right = np.maximum(b[0], c[0]), np.maximum(b[1], c[1]), np.minimum(b[2], c[2]), np.minimum(b[3], c[3])
    ai = np.maximum(bottom - top, F(0)) * np.maximum(right - left, F(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        return F(ai / (((b[2] - b[0]) * (b[3] - b[1]) + (c[2] - c[0]) * (c[3] - c[1])) - ai))


def _nms_finish(name, box, prob, l_end, nms_thresh, **extra):
    box, prob = np.ascontiguousarray(box, F), np.ascontiguousarray(prob, F)
    want = ref.keep_lists(box, prob, NMS_N_CLASS, 1, l_end, NMS_SCORE_THRESH, nms_thresh)
    return dict(name=name, box=box, prob=prob, n_class=NMS_N_CLASS, l_begin=1, l_end=l_end, score_thresh=NMS_SCORE_THRESH,
                nms_thresh=nms_thresh, want=want, **extra)


def _nms_grid(R, l_end):
    rs = np.random.RandomState(2 * R + l_end)
    c = rs.uniform(0, 400, (R, 2)); hw = np.exp(rs.uniform(np.log(4), np.log(120), (R, 2)))
    box = np.concatenate([c - hw / 2, c + hw / 2], 1).astype(F)
    rows = rs.permutation(R)
    n_dup, n_at = int(round(0.1 * R)), int(round(0.05 * R))
    box[rows[:n_dup]] = box[rows[n_dup + rs.randint(0, R - n_dup, n_dup)]]     # exact duplicates of rows that stay as they are
    prob = (rs.randint(17, 65, (R, NMS_N_CLASS)) / 64.0).astype(F)            # every score above the threshold 16 / 64
    rows = rs.permutation(R)
    prob[rows[:n_at], 2] = F(NMS_SCORE_THRESH)                                # exactly on it: not a candidate
    prob[rows[n_at:2 * n_at], 2] = (rs.randint(0, 16, n_at) / 64.0).astype(F)  # and as many below
    prob[:, 3] = (rs.randint(0, 17, R) / 64.0).astype(F)                      # no candidate
    return _nms_finish('grid-R%d-e%d' % (R, l_end), box, prob, l_end, 0.3, n_dup=n_dup, n_at=n_at)


def _nms_identical(l_end):
    R = 65
    rs = np.random.RandomState(31 + l_end)
    box = np.tile(np.asarray([[10.5, 20.25, 70.75, 90.5]], F), (R, 1))
    prob = (rs.randint(17, 60, (R, NMS_N_CLASS)) / 64.0).astype(F)
    prob[[3, 40, 64], 1] = F(1.0)                                             # the top score three times: row 64 survives
    prob[:, 2] = F(0.5)                                                       # one score for all: row R - 1 survives
    prob[:, 3] = F(0.125)
    prob[11, 3] = F(0.75)                                                     # a single candidate
    prob[:, 4] = (rs.randint(17, 20, R) / 64.0).astype(F)
    return _nms_finish('identical-e%d' % l_end, box, prob, l_end, 0.3)


def _nms_disjoint(l_end):
    R = 130
    rs = np.random.RandomState(41 + l_end)
    i = np.arange(R)
    y, x = 10.0 * (i // 16), 10.0 * (i % 16)
    box = np.stack([y, x, y + 8, x + 8], 1).astype(F)                          # 2 pixels apart
    prob = (rs.randint(17, 33, (R, NMS_N_CLASS)) / 64.0).astype(F)            # 16 values for 130 rows: long runs of ties
    prob[rs.rand(R) < 0.3, 2] = F(NMS_SCORE_THRESH)
    prob[:, 3] = F(0.0)
    return _nms_finish('disjoint-e%d' % l_end, box, prob, l_end, 0.3)


THRESHOLD_BOXES = dict(exact=(0, 1), below=(2, 3), above=(8, 9), zero_pair=(4, 5), normal=6, zero_inside=7)


def _nms_threshold(l_end):
    dn, up = np.nextafter(F(5), F(0)), np.nextafter(F(5), F(10))
    box = np.asarray([[0, 0, 10, 10], [0, 0, 10, 5],                           # IoU exactly 0.5: 50 / ((100 + 50) - 50)
                      [100, 0, 110, 10], [100, 0, 110, dn],                   # one ulp of x2 below it
                      [200, 200, 200, 210], [200, 200, 200, 210],             # zero area, one spot: 0 / 0
                      [300, 300, 340, 340], [310, 310, 310, 320],             # zero area inside a normal box: IoU 0
                      [400, 0, 410, 10], [400, 0, 410, up]], F)               # one ulp above it
    R = len(box)
    prob = np.zeros((R, NMS_N_CLASS), F)
    prob[:, 1] = (64 - np.arange(R)) / 64.0                                   # the first of each pair selects
    prob[:, 2] = (40 + np.arange(R)) / 64.0                                   # the second of each pair selects
    prob[:, 3] = 0.5                                                          # ties: the second of each pair selects
    prob[:, 4] = (np.asarray([20, 20, 30, 30, 16, 17, 18, 18, 64, 16]) / 64.0)
    return _nms_finish('threshold-e%d' % l_end, box, prob, l_end, 0.5)


@functools.lru_cache(maxsize=None)
def nms_case(name):
    kind, rest = name.split('-', 1)
    l_end = int(name.rsplit('-e', 1)[1])
    if kind == 'grid':
        return _nms_grid(int(rest.split('-')[0][1:]), l_end)
    return dict(identical=_nms_identical, disjoint=_nms_disjoint, threshold=_nms_threshold)[kind](l_end)


def class_nms_geometry(n):
    """What k_class_nms's loops do for n candidates: the mask words per row, and the trips of a 256-thread stride over the n rows."""
    return dict(nw=(n + 63) // 64, trips=(n + 255) // 256)


# ======================================================================================================================
# C. paste
# ======================================================================================================================
PASTE_GRID_PIXELS = 1024 * 256                      # predict.hip / tta.hip: pixels one trip of the grid-stride loop covers
PASTE_NAMES = ['S14-c4', 'S28-c96', 'S56-c1', 'big-S56-c4', 'img1x1-S14-c1', 'img1x40-S28-c4', 'img40x1-S14-c96', 'D0-S28-c96']


def _std_boxes(rs, S, H, W):
    b = [[10, 20, 11, 21],                              # 1 x 1
         [20.3, 30.6, 25.4, 39.7],                      # 5 x 9: downscale
         [30, 40, 30 + S, 40 + S],                      # S x S: identity
         [0, 0, H, W],                                  # the whole image
         [3.7, 50, 10.2, 70],                           # int(y2 - y1) = 6, int(y2) - int(y1) = 7
         [3.2, 4.7, 3.9, 60.0],                         # zero height
         [40, 10.05, 60, 10.95],                        # width 0.9: mw == 0
         [H - 1, W - 1, H, W]]                          # starts in the last row and the last column
    if 5 + 2 * S <= H and 8 + 2 * S + 1 <= W:
        b.append([5, 8, 5 + 2 * S, 8 + 2 * S + 1])      # 2S x (2S + 1)
    for _ in range(2):
        y0, x0 = rs.uniform(0, H - 30), rs.uniform(0, W - 30)
        b.append([y0, x0, min(y0 + rs.uniform(5, 80), H), min(x0 + rs.uniform(5, 90), W)])
    return b


def _paste_inputs(name):
    S, Cm = (int(v) for v in re.search(r'S(\d+)-c(\d+)$', name).groups())
    rs = np.random.RandomState(sum(map(ord, name)))
    if name.startswith('big'):
        size = (513, 512)
        bbox = [[100, 50, 107, 350],                    # 7 x 300
                [200.5, 20.25, 200.5 + 2 * S, 20.25 + 2 * S + 1],          # 2S x (2S + 1)
                [500, 200, 513, 512]]                   # the last rows: pixels past 262,144, y2 == H, x2 == W
    elif name.startswith('img1x1'):
        size, bbox = (1, 1), [[0, 0, 1, 1], [0, 0, 0.5, 1], [0, 0, 1, 0.9]]
    elif name.startswith('img1x40'):
        size, bbox = (1, 40), [[0, 0, 1, 40], [0, 5.5, 1, 20.2], [0, 39, 1, 40], [0.25, 3, 0.75, 30]]
    elif name.startswith('img40x1'):
        size, bbox = (40, 1), [[0, 0, 40, 1], [5.5, 0, 20.2, 1], [39, 0, 40, 1], [3, 0.25, 30, 0.75]]
    elif name.startswith('D0'):
        size, bbox = (97, 131), []
    else:
        size = (97, 131)
        bbox = _std_boxes(rs, S, *size)
    D = len(bbox)
    logits = (rs.standard_normal((D, S, S, Cm)) * 2).astype(F)
    label = rs.randint(0, Cm, D).astype(np.int32)
    if D >= 2:
        label[0], label[1] = 0, Cm - 1
    return S, Cm, size, logits, label, np.asarray(bbox, F).reshape(D, 4)


@functools.lru_cache(maxsize=None)
def paste_case(name):
    S, Cm, size, logits, label, bbox = _paste_inputs(name)
    D = len(bbox)
    sel = logits[np.arange(D), :, :, label] if D else np.zeros((0, S, S), F)          # (D,S,S): channel label[d]
    prob = ref.sigmoid_f32(sel)                                                    # mask_paste_prob's input
    c = dict(name=name, S=S, Cm=Cm, size=size, logits=logits, label=label, bbox=bbox, prob_map=prob)
    for key, maps, from_logits in (('logit', sel, True), ('prob', prob, False)):
        r64, r32 = ref.paste(maps, bbox, size, from_logits), ref.paste_f32(maps, bbox, size, from_logits)
        band, worst = pj.paste_band(r64, r32)
        n_in, n_band = pj.paste_counts(r64, band)
        c[key] = dict(ref64=r64, ref32=r32, band=band, worst=worst, n_in=n_in, n_band=n_band)
    return c


# ======================================================================================================================
# D. keypoint decode
# ======================================================================================================================
KEYPOINT_S = [7, 14, 28, 56]
KEYPOINT_KC = [(4, 4), (5, 8), (17, 32), (33, 64), (256, 256)]
KEYPOINT_SHAPES = ([(S, K, Cp, D) for S in KEYPOINT_S for K, Cp in KEYPOINT_KC for D in (1, 3) if not (K == 256 and S == 56 and D == 3)] +
                   [(14, 17, 32, 300)])


def keypoint_geometry(D, S, K):
    """csrc/keypoints.hip's launch rule: the lanes per cell P (a power of two >= ceil(K / 4)) and the number of splits of the S * S cells."""
    P = 1
    while 4 * P < K:
        P <<= 1
    step = 256 // P
    return dict(P=P, nsplit=int(max(1, min((2048 + D - 1) // max(D, 1), max(1, S * S // (step * 2))))))


@functools.lru_cache(maxsize=None)
def keypoint_case(S, K, Cp, D):
    rs = np.random.RandomState(((S * 31 + K) * 31 + Cp) * 31 + D)
    heat = (rs.standard_normal((D, S, S, Cp)) * 4).astype(F)
    heat[..., K:] = 1e4                                              # padding channels must not be read into the result
    for d in range(D):                                               # planted ties: the maximum again at later cells
        for k in range(K):
            cells = rs.randint(0, S * S - 1, 3)
            v = F(20 + rs.randint(0, 3))
            for ci in sorted(cells):
                heat[d, ci // S, ci % S, k] = v
    heat[0, :, :, 0] = 1.5                                           # all cells equal: index 0, prob 1 / S^2
    y0, x0 = rs.uniform(0, 440, D), rs.uniform(0, 600, D)
    bbox = np.stack([y0, x0, np.minimum(y0 + rs.uniform(3, 400, D), 480), np.minimum(x0 + rs.uniform(3, 400, D), 640)], 1).astype(F)
    return dict(S=S, K=K, Cp=Cp, D=D, heat=heat, bbox=bbox, want=ref.keypoint_decode(heat, bbox, K), **keypoint_geometry(D, S, K))
