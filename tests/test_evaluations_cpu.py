"""Validation mAP on the host (chainer_maskrcnn/evaluations.py, evaluator.py, train.py --eval-interval) without a device:

* a NumPy restatement of ChainerCV's mask_iou, calc_instance_segmentation_voc_prec_rec and calc_detection_voc_ap, written here
  and pinned by hand-worked cases with known answers;
* evaluations.py's matching and AP equal the restatement on random cases (distinct scores, precomputed IoU);
* the host argument checks of mrcnn_mask_iou_counts_u8 / mrcnn_mask_iou_workspace_bytes through ctypes (nothing is launched);
* the evaluator's dataset adapters and train.py's refusal of keypoint and multi-rank evaluation."""
import ctypes
import os
import sys
from collections import defaultdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

from chainer_maskrcnn import evaluations  # noqa: E402


# ---- restatement of ChainerCV (chainercv/utils/mask/mask_iou.py, chainercv/evaluations/eval_instance_segmentation_voc.py,
# ---- chainercv/evaluations/eval_detection_voc.py: calc_detection_voc_ap) ------------------------------------------------------
def ref_mask_iou(a, b):
    iou = np.empty((len(a), len(b)), dtype=np.float64)
    for n, ma in enumerate(a):
        for k, mb in enumerate(b):
            iou[n, k] = np.bitwise_and(ma, mb).sum() / np.bitwise_or(ma, mb).sum()
    return iou


def ref_prec_rec(pred_labels, pred_scores, gt_labels, gt_difficults, iou_of, iou_thresh=0.5):
    """iou_of(image, pred_index_array, gt_index_array) -> IoU of those predictions and ground truths."""
    n_pos, score, match = defaultdict(int), defaultdict(list), defaultdict(list)
    for n, (pl, ps, gl, gd) in enumerate(zip(pred_labels, pred_scores, gt_labels, gt_difficults)):
        if gd is None:
            gd = np.zeros(gl.shape[0], dtype=bool)
        for l in np.unique(np.concatenate((pl, gl)).astype(int)):
            pidx = np.flatnonzero(pl == l)
            order = ps[pidx].argsort()[::-1]
            pidx = pidx[order]
            gidx = np.flatnonzero(gl == l)
            gd_l = gd[gidx]
            n_pos[l] += np.logical_not(gd_l).sum()
            score[l].extend(ps[pidx])
            if len(pidx) == 0:
                continue
            if len(gidx) == 0:
                match[l].extend((0,) * len(pidx))
                continue
            iou = iou_of(n, pidx, gidx)
            gt_index = iou.argmax(axis=1)
            gt_index[iou.max(axis=1) < iou_thresh] = -1
            selec = np.zeros(len(gidx), dtype=bool)
            for g in gt_index:
                if g >= 0:
                    if gd_l[g]:
                        match[l].append(-1)
                    else:
                        match[l].append(1 if not selec[g] else 0)
                    selec[g] = True
                else:
                    match[l].append(0)
    n_fg = max(n_pos.keys()) + 1
    prec, rec = [None] * n_fg, [None] * n_fg
    for l in n_pos.keys():
        s = np.array(score[l])
        m = np.array(match[l], dtype=np.int8)[s.argsort()[::-1]]
        tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            prec[l] = tp / (fp + tp)
        if n_pos[l] > 0:
            rec[l] = tp / n_pos[l]
    return prec, rec


def ref_ap(prec, rec, use_07_metric=False):
    ap = np.empty(len(prec))
    for l in range(len(prec)):
        if prec[l] is None or rec[l] is None:
            ap[l] = np.nan
            continue
        if use_07_metric:
            ap[l] = 0
            for t in np.arange(0., 1.1, 0.1):
                p = 0 if np.sum(rec[l] >= t) == 0 else np.max(np.nan_to_num(prec[l])[rec[l] >= t])
                ap[l] += p / 11
        else:
            mpre = np.concatenate(([0], np.nan_to_num(prec[l]), [0]))
            mrec = np.concatenate(([0], rec[l], [1]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            i = np.where(mrec[1:] != mrec[:-1])[0]
            ap[l] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


def ref_eval(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults=None, iou_thresh=0.5, use_07_metric=False):
    if gt_difficults is None:
        gt_difficults = [None] * len(gt_labels)
    iou_of = lambda n, p, g: ref_mask_iou(pred_masks[n][p], gt_masks[n][g])
    prec, rec = ref_prec_rec(pred_labels, pred_scores, gt_labels, gt_difficults, iou_of, iou_thresh)
    ap = ref_ap(prec, rec, use_07_metric)
    with _quiet():
        m = np.nanmean(ap)
    return {'ap': ap, 'map': m}


class _quiet(object):
    def __enter__(self):
        import warnings
        self.w = warnings.catch_warnings()
        self.w.__enter__()
        warnings.simplefilter('ignore')

    def __exit__(self, *a):
        self.w.__exit__(*a)


def _box(H, W, y0, x0, y1, x1):
    m = np.zeros((H, W), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def _ious(pred_masks, gt_masks):
    return [ref_mask_iou(p, g) if len(p) and len(g) else np.zeros((len(p), len(g))) for p, g in zip(pred_masks, gt_masks)]


def _ours(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults=None, use_07_metric=False):
    prec, rec = evaluations.calc_prec_rec_from_iou(_ious(pred_masks, gt_masks), pred_labels, pred_scores, gt_labels, gt_difficults)
    ap = evaluations.calc_detection_voc_ap(prec, rec, use_07_metric)
    return {'ap': ap, 'map': evaluations.nanmean(ap)}


# ---- hand-worked cases ---------------------------------------------------------------------------------------------------------
def _case_tp_dup_miss():
    """class 0: gt g0 (top-left 2x2), g1 (bottom-right 2x2); p0 = g0 (IoU 1, score .9), p1 = g0 + 1 pixel (IoU .8 with the taken g0,
    score .8): matches [1, 0], prec [1, .5], rec [.5, .5]; g1 is missed."""
    g = np.stack([_box(4, 4, 0, 0, 2, 2), _box(4, 4, 2, 2, 4, 4)])
    p1 = _box(4, 4, 0, 0, 2, 2)
    p1[2, 0] = True
    p = np.stack([_box(4, 4, 0, 0, 2, 2), p1])
    return [p], [np.array([0, 0])], [np.array([.9, .8], np.float32)], [g], [np.array([0, 0])]


def test_restatement_tp_duplicate_and_miss():
    pm, pl, ps, gm, gl = _case_tp_dup_miss()
    np.testing.assert_allclose(ref_mask_iou(pm[0], gm[0]), [[1, 0], [.8, 0]])
    prec, rec = ref_prec_rec(pl, ps, gl, [None], lambda n, a, b: ref_mask_iou(pm[n][a], gm[n][b]))
    np.testing.assert_allclose(prec[0], [1, .5])
    np.testing.assert_allclose(rec[0], [.5, .5])
    # area under the interpolated curve: recall 0 -> .5 at precision 1, .5 -> 1 at precision 0
    assert ref_eval(pm, pl, ps, gm, gl)['ap'][0] == pytest.approx(0.5)
    # 11-point: the thresholds 0, .1, ..., .5 reach precision 1, the five above reach nothing
    assert ref_eval(pm, pl, ps, gm, gl, use_07_metric=True)['ap'][0] == pytest.approx(6. / 11)
    for use07, want in ((False, 0.5), (True, 6. / 11)):
        r = _ours(pm, pl, ps, gm, gl, use_07_metric=use07)
        assert r['ap'][0] == pytest.approx(want) and r['map'] == pytest.approx(want)


def test_restatement_difficult_ground_truth_is_not_counted():
    """class 0: g0 difficult, g1 not; p0 (score .9) hits g0 -> -1, p1 (score .5) hits g1 -> 1: prec [nan, 1], rec [0, 1], AP 1."""
    g = np.stack([_box(4, 6, 0, 0, 2, 2), _box(4, 6, 2, 3, 4, 6)])
    p = g.copy()
    args = ([p], [np.array([0, 0])], [np.array([.9, .5], np.float32)], [g], [np.array([0, 0])], [np.array([True, False])])
    prec, rec = ref_prec_rec(args[1], args[2], args[4], args[5], lambda n, a, b: ref_mask_iou(p[a], g[b]))
    assert np.isnan(prec[0][0]) and prec[0][1] == 1
    np.testing.assert_allclose(rec[0], [0, 1])
    assert ref_eval(*args)['ap'][0] == pytest.approx(1.0)
    acc = evaluations.VOCMatchAccumulator()
    acc.add_image(ref_mask_iou(p, g), args[1][0], args[2][0], args[4][0], args[5][0])
    assert acc.match[0] == [-1, 1] and acc.n_pos[0] == 1
    assert _ours(*args)['ap'][0] == pytest.approx(1.0)


def test_restatement_class_without_ground_truth_is_nan_and_left_out():
    """class 1: one exact hit (AP 1); class 2: a prediction but no ground truth (nan, excluded); class 0: neither (nan)."""
    g = np.stack([_box(4, 4, 0, 0, 2, 2)])
    p = np.stack([_box(4, 4, 0, 0, 2, 2), _box(4, 4, 2, 2, 4, 4)])
    args = ([p], [np.array([1, 2])], [np.array([.7, .9], np.float32)], [g], [np.array([1])])
    for r in (ref_eval(*args), _ours(*args)):
        assert np.isnan(r['ap'][0]) and r['ap'][1] == pytest.approx(1.0) and np.isnan(r['ap'][2])
        assert r['map'] == pytest.approx(1.0)


def test_restatement_prediction_below_threshold_is_a_false_positive():
    """IoU 4/8 = .5 is a hit; IoU 4/10 < .5 makes the prediction a false positive and the ground truth a miss: AP 0."""
    g = np.stack([_box(4, 5, 0, 0, 2, 2)])
    p = np.stack([_box(4, 5, 0, 0, 2, 4)])            # 8 pixels, 4 of them g0's
    assert ref_mask_iou(p, g)[0, 0] == pytest.approx(0.5)
    assert _ours([p], [np.array([0])], [np.array([.5], np.float32)], [g], [np.array([0])])['ap'][0] == pytest.approx(1.0)
    p[0, 2, 0:2] = True                                  # 10 pixels: IoU .4 -> no match
    args = ([p], [np.array([0])], [np.array([.5], np.float32)], [g], [np.array([0])])
    assert ref_mask_iou(p, g)[0, 0] == pytest.approx(0.4)
    for r in (ref_eval(*args), _ours(*args)):
        assert r['ap'][0] == 0 and r['map'] == 0
    acc = evaluations.VOCMatchAccumulator()
    acc.add_image(ref_mask_iou(p, g), args[1][0], args[2][0], args[4][0])
    assert acc.match[0] == [0]


def test_iou_from_counts_equals_the_restatement():
    rs = np.random.RandomState(0)
    a = rs.rand(7, 9, 11) < 0.4
    b = rs.rand(5, 9, 11) < 0.6
    b[0] = a[2]
    inter = np.array([[np.logical_and(x, y).sum() for y in b] for x in a])
    got = evaluations.iou_from_counts(inter, a.reshape(7, -1).sum(1), b.reshape(5, -1).sum(1))
    np.testing.assert_array_equal(got, ref_mask_iou(a, b))
    assert got[2, 0] == 1.0
    assert np.isnan(evaluations.iou_from_counts(np.zeros((1, 1)), [0], [0])[0, 0])         # two empty masks: 0 / 0, as in ChainerCV


@pytest.mark.parametrize('seed', range(12))
@pytest.mark.parametrize('use_07_metric', [False, True])
def test_matching_and_ap_equal_the_restatement_on_random_cases(seed, use_07_metric):
    rs = np.random.RandomState(seed)
    n_img, n_class = 6, 5
    pl, ps, gl, gd, ious = [], [], [], [], []
    scores = rs.permutation(1000)[:n_img * 40].astype(np.float32) / 1000.      # distinct over the whole set
    k = 0
    for _ in range(n_img):
        D, G = rs.randint(0, 25), rs.randint(0, 8)
        pl.append(rs.randint(0, n_class, D))
        ps.append(scores[k:k + D])
        k += D
        gl.append(rs.randint(0, n_class, G))
        gd.append(rs.rand(G) < 0.15)
        iou = rs.rand(D, G)
        iou[rs.rand(D, G) < 0.3] = 0
        ious.append(iou)
    want_prec, want_rec = ref_prec_rec(pl, ps, gl, gd, lambda n, p, g: ious[n][np.ix_(p, g)], 0.5)
    prec, rec = evaluations.calc_prec_rec_from_iou(ious, pl, ps, gl, gd, iou_thresh=0.5)
    assert len(prec) == len(want_prec)
    for a, b in zip(prec + rec, want_prec + want_rec):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b)
    want = ref_ap(want_prec, want_rec, use_07_metric)
    got = evaluations.calc_detection_voc_ap(prec, rec, use_07_metric)
    np.testing.assert_array_equal(got, want)
    with _quiet():
        assert evaluations.nanmean(got) == pytest.approx(np.nanmean(want), nan_ok=True)


def test_equal_scores_keep_input_order():
    """The documented tie rule: of two predictions with the same score, the earlier one is taken first (and gets the match)."""
    acc = evaluations.VOCMatchAccumulator()
    acc.add_image(np.array([[0.9], [0.8]]), np.array([0, 0]), np.array([.5, .5], np.float32), np.array([0]))
    assert acc.match[0] == [1, 0]
    acc.add_image(np.array([[0.6]]), np.array([0]), np.array([.5], np.float32), np.array([0]))
    prec, rec = acc.prec_rec()
    np.testing.assert_allclose(prec[0], [1, .5, 2. / 3])


# ---- C entry points: host argument checks (no launch) ---------------------------------------------------------------------------
def _lib():
    from chainer_maskrcnn import _hip
    return _hip.lib()


def test_workspace_query():
    lib = _lib()
    assert lib.mrcnn_mask_iou_workspace_bytes(100, 20, 375 * 500) == 120 * ((375 * 500 + 63) // 64) * 8
    assert lib.mrcnn_mask_iou_workspace_bytes(1, 1, 1) == 16
    assert lib.mrcnn_mask_iou_workspace_bytes(0, 0, 1 << 20) == 0
    assert lib.mrcnn_mask_iou_workspace_bytes(4, 0, 1024 * 1024) == 4 * 16384 * 8
    assert lib.mrcnn_mask_iou_workspace_bytes(-1, 2, 64) == 0 and lib.mrcnn_mask_iou_workspace_bytes(1, 2, -64) == 0
    # 64-bit sizes: (2^16 masks of 2^20 pixels) = 2^36 / 64 words
    assert lib.mrcnn_mask_iou_workspace_bytes(1 << 15, 1 << 15, 1 << 20) == (1 << 16) * (1 << 14) * 8


def test_argument_errors_are_reported_before_any_launch():
    lib = _lib()
    buf = (ctypes.c_char * 4096)()
    P = ctypes.cast(buf, ctypes.c_void_p)            # non-null stand-ins: every call below must be rejected before a launch
    N = None
    ws = lib.mrcnn_mask_iou_workspace_bytes(3, 2, 100)

    def call(a=P, Da=3, la=N, b=P, Db=2, lb=N, HW=100, w=P, wb=ws, inter=P, aa=P, ab=P):
        return lib.mrcnn_mask_iou_counts_u8(a, Da, la, b, Db, lb, HW, w, wb, inter, aa, ab, N)

    for kw in (dict(Da=-1), dict(Db=-2), dict(HW=-5)):
        assert call(**kw) == -1 and b'negative' in lib.mrcnn_last_error()
    assert call(la=P) == -1 and b'label' in lib.mrcnn_last_error()
    assert call(lb=P) == -1
    for kw in (dict(a=N), dict(b=N), dict(inter=N), dict(aa=N), dict(ab=N)):
        assert call(**kw) == -1, kw
    assert call(wb=ws - 1) == -3 and b'workspace' in lib.mrcnn_last_error()
    assert call(w=N) == -3
    # an empty side needs neither its masks nor the intersections; the workspace check still applies to the other side
    assert call(Db=0, b=N, inter=N, ab=N, wb=lib.mrcnn_mask_iou_workspace_bytes(3, 0, 100) - 8) == -3
    assert call(Da=0, a=N, inter=N, aa=N, wb=0) == -3
    # nothing at all to do: returns 0 without touching a device
    assert lib.mrcnn_mask_iou_counts_u8(N, 0, N, N, 0, N, 100, N, 0, N, N, N, N) == 0


def test_op_has_no_cpu_fallback():
    import torch
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    with pytest.raises(_hip.MrcnnHipError):
        ops.mask_iou_counts(torch.zeros(2, 4, 4, dtype=torch.bool), torch.zeros(3, 4, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.mask_iou_counts(torch.zeros(2, 4, 4, dtype=torch.bool), torch.zeros(3, 4, 4, dtype=torch.bool), a_label=torch.zeros(2))


# ---- evaluator plumbing --------------------------------------------------------------------------------------------------------
def test_coco_example_adapter_and_synthetic_split():
    from chainer_maskrcnn.evaluator import SyntheticEvalDataset, TransformedDataset, coco_mask_example
    img = np.zeros((3, 5, 7), np.float32)
    m = [np.eye(5, 7, dtype=np.uint8), np.ones((5, 7), np.uint8)]
    i2, gm, gl = coco_mask_example((img, np.zeros((2, 4)), np.array([3, 4]), m))
    assert i2 is not None and gm.shape == (2, 5, 7) and gl.dtype == np.int32 and list(gl) == [3, 4]
    _, gm0, gl0 = coco_mask_example((img, np.zeros((0, 4)), np.zeros((0,), np.int32), []))
    assert gm0.shape == (0, 5, 7) and gl0.shape == (0,)
    td = TransformedDataset([(img, None, [1], [m[0]])] * 5, coco_mask_example, n=2)
    assert len(td) == 2 and td[1][1].shape == (1, 5, 7)
    with pytest.raises(IndexError):
        td[2]
    ds = SyntheticEvalDataset(3, 64, 80, n_fg_class=80)
    a, b = ds[1], SyntheticEvalDataset(3, 64, 80)[1]
    assert len(ds) == 3 and a[0].shape == (3, 64, 80) and a[1].shape == (8, 64, 80) and a[2].shape == (8,)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[0].max() > 1.0                              # 0..255, the scale predict() takes
    import train
    from chainer_maskrcnn.utils.synthetic import make_batch
    train_imgs = [make_batch(j + 1, 1, 64, 80)['imgs'] for j in range(8)]            # the training pool's seeds (world 1)
    assert not any(np.array_equal(ds[i][0] / 255, t[0]) for i in range(3) for t in train_imgs)
    assert train.build_parser().parse_args([]).eval_interval == 0                      # off by default


def test_train_refuses_keypoint_and_multi_rank_evaluation(monkeypatch):
    import train
    a = train.build_parser(keypoints=True).parse_args(['--eval-interval', '5'])
    with pytest.raises(ValueError, match='mask heads only'):
        train.run(a, keypoints=True)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='multi-GPU'):
        train.run(train.build_parser().parse_args(['--eval-interval', '5']))
