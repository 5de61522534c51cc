"""COCO keypoint AP on the host (chainer_maskrcnn/evaluations.py keypoint part, evaluator.py, train.py --eval-metric) without a device:

* a literal restatement of pycocotools' COCOeval for iouType='keypoints' (computeOks, evaluateImg, accumulate, summarize over
  dicts, as written there), pinned by hand-worked cases;
* the streaming COCOKeypointMatchAccumulator equals the restatement on random data;
* COCOKeypointsLoader.get_annotations on a small hand-written person_keypoints file;
* the host argument checks of mrcnn_keypoint_decode_f32 through ctypes (nothing is launched);
* train.py's --eval-metric flag and its refusals."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

from chainer_maskrcnn import evaluations  # noqa: E402

ONE = pytest.approx(1.0, abs=1e-12)        # precision tp / (fp + tp + eps): a perfect score is 1 - 2e-16
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


# ---- restatement of pycocotools/cocoeval.py (COCOeval with iouType='keypoints', one category) and coco.py loadRes -------------------
def _ref_compute_oks(gts, dts, sigmas, max_det):
    inds = np.argsort([-d['score'] for d in dts], kind='mergesort')
    dts = [dts[i] for i in inds]
    if len(dts) > max_det:
        dts = dts[0:max_det]
    if len(gts) == 0 or len(dts) == 0:
        return []
    ious = np.zeros((len(dts), len(gts)))
    vars = (sigmas * 2) ** 2
    k = len(sigmas)
    for j, gt in enumerate(gts):
        g = np.array(gt['keypoints'])
        xg = g[0::3]
        yg = g[1::3]
        vg = g[2::3]
        k1 = np.count_nonzero(vg > 0)
        bb = gt['bbox']
        x0 = bb[0] - bb[2]
        x1 = bb[0] + bb[2] * 2
        y0 = bb[1] - bb[3]
        y1 = bb[1] + bb[3] * 2
        for i, dt in enumerate(dts):
            d = np.array(dt['keypoints'])
            xd = d[0::3]
            yd = d[1::3]
            if k1 > 0:
                dx = xd - xg
                dy = yd - yg
            else:
                z = np.zeros((k))
                dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
            e = (dx ** 2 + dy ** 2) / vars / (gt['area'] + np.spacing(1)) / 2
            if k1 > 0:
                e = e[vg > 0]
            ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
    return ious


def _ref_evaluate_img(gt, dt, ious, a_rng, max_det, iou_thrs):
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        g['_ignore'] = 1 if (g['ignore'] or (g['area'] < a_rng[0] or g['area'] > a_rng[1])) else 0
    gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(o['iscrowd']) for o in gt]
    ious = ious[:, gtind] if len(ious) > 0 else ious
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gtIg = np.array([g['_ignore'] for g in gt])
    dtIg = np.zeros((T, D))
    if not len(ious) == 0:
        for tind, t in enumerate(iou_thrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = gt[m]['id']
                gtm[tind, m] = d['id']
    a = np.array([d['area'] < a_rng[0] or d['area'] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {'dtMatches': dtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}


def _ref_accumulate(eval_imgs, n_area, max_det, iou_thrs, rec_thrs):
    T, R = len(iou_thrs), len(rec_thrs)
    precision = -np.ones((T, R, n_area))
    recall = -np.ones((T, n_area))
    for a in range(n_area):
        E = [e[a] for e in eval_imgs]
        E = [e for e in E if e is not None]
        if len(E) == 0:
            continue
        dtScores = np.concatenate([e['dtScores'][0:max_det] for e in E])
        inds = np.argsort(-dtScores, kind='mergesort')
        dtm = np.concatenate([e['dtMatches'][:, 0:max_det] for e in E], axis=1)[:, inds]
        dtIg = np.concatenate([e['dtIgnore'][:, 0:max_det] for e in E], axis=1)[:, inds]
        gtIg = np.concatenate([e['gtIgnore'] for e in E])
        npig = np.count_nonzero(gtIg == 0)
        if npig == 0:
            continue
        tps = np.logical_and(dtm, np.logical_not(dtIg))
        fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
        tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
        fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
        for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
            tp = np.array(tp)
            fp = np.array(fp)
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            q = np.zeros((R,))
            recall[t, a] = rc[-1] if nd else 0
            pr = pr.tolist()
            q = q.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            inds_r = np.searchsorted(rc, rec_thrs, side='left')
            try:
                for ri, pi in enumerate(inds_r):
                    q[ri] = pr[pi]
            except IndexError:
                pass
            precision[t, :, a] = np.array(q)
    return precision, recall


def _ref_summarize(precision, recall, iou_thrs):
    def s(ap, t=None, a=0):
        x = precision if ap else recall
        if t is not None:
            x = x[np.where(np.isclose(iou_thrs, t))[0]]
        x = x[..., a]
        return -1 if len(x[x > -1]) == 0 else float(np.mean(x[x > -1]))
    return {'AP': s(1), 'AP50': s(1, .5), 'AP75': s(1, .75), 'APm': s(1, a=1), 'APl': s(1, a=2),
            'AR': s(0), 'AR50': s(0, .5), 'AR75': s(0, .75), 'ARm': s(0, a=1), 'ARl': s(0, a=2)}


def ref_coco_keypoint_eval(dt_yx, dt_scores, gt_kp_yxv, gt_areas, gt_crowds, gt_bboxes, sigmas=SIGMAS, max_det=20):
    """COCOeval over per-image arrays: the results are turned into COCO's dicts ((x, y, v) keypoint lists, loadRes's area and ids,
    _prepare's ignore flag) and evaluated as pycocotools does."""
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    a_rngs = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    eval_imgs, did, gid = [], 0, 0
    for dyx, ds, gk, ga, gc, gb in zip(dt_yx, dt_scores, gt_kp_yxv, gt_areas, gt_crowds, gt_bboxes):
        dts, gts = [], []
        for p, sc in zip(np.asarray(dyx, np.float64), np.asarray(ds, np.float64)):
            did += 1
            x, y = p[:, 1], p[:, 0]
            kp = np.stack([x, y, np.ones_like(x)], 1).reshape(-1).tolist()
            dts.append({'keypoints': kp, 'score': float(sc), 'id': did, 'area': (x.max() - x.min()) * (y.max() - y.min())})
        for g, a, c, b in zip(np.asarray(gk, np.float64), np.asarray(ga, np.float64), np.asarray(gc), np.asarray(gb, np.float64)):
            gid += 1
            nk = int(np.count_nonzero(g[:, 2] > 0))
            gts.append({'keypoints': g[:, [1, 0, 2]].reshape(-1).tolist(), 'area': float(a), 'iscrowd': int(bool(c)), 'id': gid,
                        'bbox': b.tolist(), 'num_keypoints': nk, 'ignore': bool(c) or nk == 0})
        ious = _ref_compute_oks(gts, dts, sigmas, max_det)
        eval_imgs.append([_ref_evaluate_img([dict(g) for g in gts], dts, ious, r, max_det, iou_thrs) for r in a_rngs])
    precision, recall = _ref_accumulate(eval_imgs, len(a_rngs), max_det, iou_thrs, rec_thrs)
    return _ref_summarize(precision, recall, iou_thrs)


# ---- hand-worked cases -----------------------------------------------------------------------------------------------------------------
def _gt(yx, v=2):
    return np.concatenate([np.asarray(yx, np.float64), np.full(np.asarray(yx).shape[:-1] + (1,), v, np.float64)], -1)


def _both(dt, sc, gk, ga, gc, gb):
    got = evaluations.eval_keypoint_coco(dt, sc, gk, ga, gc, gb)
    want = ref_coco_keypoint_eval(dt, sc, gk, ga, gc, gb)
    assert got == want, (got, want)
    return got


def test_oks_perfect_match_and_known_offset():
    rs = np.random.RandomState(0)
    gt_yx = rs.rand(1, 17, 2) * 100
    gt = _gt(gt_yx)
    area = np.array([2500.0])
    box = np.array([[0, 0, 100, 100.]])
    assert evaluations.keypoint_oks(gt_yx, gt, area, box)[0, 0] == 1.0
    d = 3.0
    dt = gt_yx.copy()
    dt[0, :, 1] += d                                             # every keypoint d to the right
    want = np.mean(np.exp(-d * d / (2 * (area[0] + np.spacing(1)) * (2 * SIGMAS) ** 2)))
    np.testing.assert_allclose(evaluations.keypoint_oks(dt, gt, area, box)[0, 0], want, rtol=1e-14)
    only = _gt(gt_yx)
    only[0, 5:, 2] = 0                                           # only the first 5 keypoints labelled: the others do not count
    dt2 = dt.copy()
    dt2[0, 5:] += 50
    want5 = np.mean(np.exp(-d * d / (2 * (area[0] + np.spacing(1)) * (2 * SIGMAS[:5]) ** 2)))
    np.testing.assert_allclose(evaluations.keypoint_oks(dt2, only, area, box)[0, 0], want5, rtol=1e-14)
    np.testing.assert_allclose(evaluations.keypoint_oks(dt2, only, area, box), _ref_compute_oks(
        [{'keypoints': only[0][:, [1, 0, 2]].reshape(-1).tolist(), 'area': 2500.0, 'bbox': [0, 0, 100, 100.]}],
        [{'keypoints': np.concatenate([dt2[0][:, [1, 0]], np.ones((17, 1))], 1).reshape(-1).tolist(), 'score': 1.}], SIGMAS, 20),
        rtol=1e-15)


def test_oks_without_labelled_keypoints_measures_to_the_expanded_box():
    gt = np.zeros((1, 17, 3))                                     # v = 0 everywhere
    box = np.array([[10., 20., 30., 40.]])                        # x, y, w, h -> x in [-20, 70], y in [-20, 100]
    area = np.array([900.0])
    inside = np.zeros((1, 17, 2))
    inside[0, :, 0], inside[0, :, 1] = 100.0, 70.0               # (y, x) inside the expanded box: distance 0
    assert evaluations.keypoint_oks(inside, gt, area, box)[0, 0] == 1.0
    out = inside.copy()
    out[0, :, 1] = 75.0                                           # 5 right of x1 = 70
    want = np.mean(np.exp(-25.0 / (2 * (900.0 + np.spacing(1)) * (2 * SIGMAS) ** 2)))
    np.testing.assert_allclose(evaluations.keypoint_oks(out, gt, area, box)[0, 0], want, rtol=1e-14)
    below = inside.copy()
    below[0, :, 0] = -23.0                                        # 3 above y0 = -20, inside in x
    want = np.mean(np.exp(-9.0 / (2 * (900.0 + np.spacing(1)) * (2 * SIGMAS) ** 2)))
    np.testing.assert_allclose(evaluations.keypoint_oks(below, gt, area, box)[0, 0], want, rtol=1e-14)


def _person(rs, cy, cx, n=1, size=60.0):
    return rs.rand(n, 17, 2) * size + [cy, cx]


def test_crowd_ground_truth_absorbs_several_detections():
    rs = np.random.RandomState(1)
    g = _gt(_person(rs, 0, 0, 2))
    area, crowd = np.array([5000., 5000.]), np.array([False, True])
    box = np.array([[0, 0, 60, 60.]] * 2)
    dt = np.stack([g[1, :, :2], g[1, :, :2], g[1, :, :2], g[0, :, :2]])   # three on the crowd, then the true positive
    r = _both([dt], [np.array([.9, .8, .7, .6])], [g], [area], [crowd], [box])
    assert r['AP'] == ONE and r['AR'] == 1.0                      # the three on the crowd are ignored, not false positives
    r2 = _both([dt], [np.array([.9, .8, .7, .6])], [g], [area], [np.array([False, False])], [box])
    # without the crowd flag: hit, miss, miss, hit -> precision 1 up to recall .5 (51 points), 2/4 up to recall 1 (50 points)
    assert r2['AR'] == 1.0 and r2['AP'] == pytest.approx((51 * 1.0 + 50 * 0.5) / 101, abs=1e-12)


def test_ignored_ground_truth_turns_a_false_positive_into_an_ignore():
    rs = np.random.RandomState(2)
    g = _gt(_person(rs, 0, 0, 2))
    g[1, :, 2] = 0                                                # second person: no labelled keypoint (num_keypoints == 0): ignored
    area, box = np.array([5000., 5000.]), np.array([[0, 0, 60, 60.]] * 2)
    near_ignored = g[1, :, :2] + 0.0                              # a detection that only the ignored person matches (box distance 0)
    far_box = np.array([[0, 0, 60, 60.], [500, 500, 60, 60.]])
    dt = np.stack([near_ignored, g[0, :, :2]])
    r = _both([dt], [np.array([.9, .8])], [g], [area], [np.zeros(2, bool)], [box])
    assert r['AP'] == ONE                                          # ignored, so the true positive keeps precision 1
    g2 = g.copy()
    g2[1, :, 2] = 2
    g2[1, :, :2] += 400                                           # now a labelled person far away: the detection is a false positive
    r2 = _both([dt], [np.array([.9, .8])], [g2], [area], [np.zeros(2, bool)], [far_box])
    assert r2['AP'] < 1.0


def test_per_image_cut_at_twenty():
    rs = np.random.RandomState(3)
    g = _gt(_person(rs, 0, 0))
    area, box = np.array([5000.]), np.array([[0, 0, 60, 60.]])
    junk = _person(rs, 300, 300, 20)
    dt = np.concatenate([junk, g[:, :, :2]])                      # the match is the 21st best: cut away
    sc = np.concatenate([np.linspace(1, .9, 20), [.5]])
    r = _both([dt], [sc], [g], [area], [np.zeros(1, bool)], [box])
    assert r['AP'] == 0.0 and r['AR'] == 0.0
    sc2 = np.concatenate([np.linspace(1, .9, 20), [.95]])        # now 11th: inside the cut
    r2 = _both([dt], [sc2], [g], [area], [np.zeros(1, bool)], [box])
    assert r2['AR'] == 1.0


def test_area_ranges():
    rs = np.random.RandomState(4)
    g = _gt(np.concatenate([_person(rs, 0, 0), _person(rs, 200, 200, size=150)]))
    box = np.array([[0, 0, 60, 60.], [200, 200, 150, 150.]])
    # (gt areas, APm, APl): closed intervals, so 32^2 and 96^2 are medium and 96^2 is large too; -1 = no ground truth in the range
    for areas, apm, apl in (((1000., 20000.), -1.0, 1.0), ((32. ** 2, 96. ** 2), 1.0, 1.0), ((96. ** 2 + 1, 96. ** 2 + 1), -1.0, 1.0),
                            ((500., 800.), -1.0, -1.0)):
        area = np.array(areas)
        r = _both([g[:, :, :2]], [np.array([.9, .8])], [g], [area], [np.zeros(2, bool)], [box])
        assert r['APm'] == (ONE if apm == 1 else apm) and r['APl'] == (ONE if apl == 1 else apl), (areas, r)
        assert r['AP'] == ONE


def test_equal_scores_keep_input_and_image_order():
    rs = np.random.RandomState(5)
    g = [_gt(_person(rs, 0, 0)), _gt(_person(rs, 0, 0))]
    area, box = np.array([5000.]), np.array([[0, 0, 60, 60.]])
    miss = _person(rs, 400, 400)
    # image 0: a miss then a hit, image 1: a hit; all scores equal.  Order miss, hit, hit: precision 0, 1/2, 2/3.
    dt = [np.concatenate([miss, g[0][:, :, :2]]), g[1][:, :, :2]]
    sc = [np.array([.5, .5]), np.array([.5])]
    r = _both(dt, sc, g, [area] * 2, [np.zeros(1, bool)] * 2, [box] * 2)
    np.testing.assert_allclose(r['AP50'], (51 * (2 / 3) + 50 * (2 / 3)) / 101, rtol=1e-12)
    dt2 = [np.concatenate([g[0][:, :, :2], miss]), g[1][:, :, :2]]      # hit first: 1, then the miss, then a hit at 2/3
    r2 = _both(dt2, sc, g, [area] * 2, [np.zeros(1, bool)] * 2, [box] * 2)
    np.testing.assert_allclose(r2['AP50'], (51 * 1.0 + 50 * (2 / 3)) / 101, rtol=1e-12)


def test_101_point_precision_by_hand():
    rs = np.random.RandomState(6)
    g = _gt(_person(rs, 0, 0, 4, size=40) + np.arange(4)[:, None, None] * 100)
    area, box = np.full(4, 5000.), np.array([[j * 100, j * 100, 40, 40.] for j in range(4)])
    miss = _person(rs, 900, 900)
    # ranked: hit, miss, hit, hit (4 ground truths): recall .25, .25, .5, .75; precision 1, 1/2, 2/3, 3/4 -> envelope 1, 3/4, 3/4, 3/4
    dt = np.concatenate([g[:1, :, :2], miss, g[1:3, :, :2]])
    r = _both([dt], [np.array([.9, .8, .7, .6])], [g], [area], [np.zeros(4, bool)], [box])
    # recall points 0..25 -> 1 (26 points), 26..75 -> 3/4 (50 points), 76..100 -> 0 (25 points)
    np.testing.assert_allclose(r['AP50'], (26 * 1.0 + 50 * 0.75) / 101, rtol=1e-12)
    assert r['AR50'] == 0.75


def test_no_ground_truth_and_no_detection():
    r = evaluations.eval_keypoint_coco([], [], [], [], [], [])
    assert all(v == -1.0 for v in r.values())
    rs = np.random.RandomState(7)
    only_dt = _both([_person(rs, 0, 0, 3)], [np.array([.9, .5, .1])], [np.zeros((0, 17, 3))], [np.zeros(0)], [np.zeros(0, bool)],
                    [np.zeros((0, 4))])
    assert only_dt['AP'] == -1.0


@pytest.mark.parametrize('seed', range(6))
def test_streaming_accumulator_equals_the_restatement_on_random_data(seed):
    rs = np.random.RandomState(100 + seed)
    dt, sc, gk, ga, gc, gb = [], [], [], [], [], []
    for _ in range(rs.randint(1, 7)):
        G, D = rs.randint(0, 6), rs.randint(0, 30)
        cen = rs.rand(max(G, 1), 2) * 400
        size = rs.uniform(20, 200, max(G, 1))
        g = np.concatenate([cen[:G, None] + rs.rand(G, 17, 2) * size[:G, None, None], rs.randint(0, 3, (G, 17, 1))], -1).astype(np.float64)
        if G:
            g[rs.rand(G) < 0.2, :, 2] = 0
        src = rs.randint(0, max(G, 1), D)
        p = (g[src, :, :2] if G else rs.rand(D, 17, 2) * 400) + rs.standard_normal((D, 17, 2)) * rs.choice([1., 5., 20.], (D, 1, 1))
        dt.append(p.astype(np.float32))
        sc.append(np.round(rs.rand(D), 1))                        # coarse scores: many ties
        gk.append(g)
        ga.append(size[:G] ** 2 * rs.uniform(.3, 1.2, G))
        gc.append(rs.rand(G) < 0.15)
        gb.append(np.concatenate([cen[:G, ::-1], np.stack([size[:G], size[:G]], 1)], 1))
    _both(dt, sc, gk, ga, gc, gb)


# ---- COCOKeypointsLoader.get_annotations -------------------------------------------------------------------------------------------
def test_get_annotations_on_a_small_person_keypoints_file(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOKeypointsLoader
    kp = lambda v: [10, 20, v] * 17
    anno = {'images': [{'id': 7, 'file_name': 'a.jpg', 'height': 50, 'width': 60}, {'id': 3, 'file_name': 'b.jpg', 'height': 50, 'width': 60},
                       {'id': 9, 'file_name': 'c.jpg', 'height': 50, 'width': 60}],
            'annotations': [{'id': 1, 'image_id': 7, 'category_id': 1, 'bbox': [1.5, 2.5, 30.25, 20.0], 'area': 410.5, 'iscrowd': 0,
                             'num_keypoints': 17, 'keypoints': kp(2), 'segmentation': [[1, 2, 30, 2, 30, 20]]},
                            {'id': 2, 'image_id': 7, 'category_id': 1, 'bbox': [0.0, 0.0, 0.5, 4.0], 'area': 1.25, 'iscrowd': 1,
                             'num_keypoints': 0, 'keypoints': kp(0), 'segmentation': {'counts': [0, 4], 'size': [50, 60]}},
                            {'id': 3, 'image_id': 3, 'category_id': 1, 'bbox': [5, 6, 7, 8], 'area': 56.0, 'iscrowd': 0,
                             'num_keypoints': 1, 'keypoints': [1, 2, 1] + [0, 0, 0] * 16, 'segmentation': [[5, 6, 12, 6, 12, 14]]}],
            'categories': [{'id': 1, 'name': 'person'}]}
    (tmp_path / 'person_keypoints_val2017.json').write_text(json.dumps(anno))
    ld = COCOKeypointsLoader(anno_dir=str(tmp_path), img_dir=str(tmp_path / 'none'), split='val', data_type='2017')
    assert len(ld) == 2                                            # image 9 has no annotation; images in ascending id: 3, 7
    a0, a1 = ld.get_annotations(0), ld.get_annotations(1)          # no image is read (img_dir does not exist)
    np.testing.assert_array_equal(a0['area'], [56.0])
    np.testing.assert_array_equal(a0['num_keypoints'], [1])
    np.testing.assert_array_equal(a1['area'], [410.5, 1.25])
    np.testing.assert_array_equal(a1['iscrowd'], [False, True])
    np.testing.assert_array_equal(a1['num_keypoints'], [17, 0])
    np.testing.assert_array_equal(a1['bbox'], [[1.5, 2.5, 30.25, 20.0], [0.0, 0.0, 0.5, 4.0]])
    assert a1['area'].dtype == np.float64 and a1['bbox'].shape == (2, 4)
    with pytest.raises(IndexError):
        ld.get_annotations(2)
    from chainer_maskrcnn.evaluator import COCOKeypointEvalDataset, coco_keypoint_example
    ld.get_example = lambda i: (np.zeros((3, 50, 60), np.float32), ld._boxes[i].copy(), ld._kps[i].copy())    # stand-in for the JPEG
    img, gt_kp, area, crowd, box = coco_keypoint_example(ld, 1)
    assert gt_kp.shape == (2, 17, 3) and (gt_kp[0, 0] == [20, 10, 2]).all()     # (x, y, v) -> (y, x, v)
    np.testing.assert_array_equal(area, a1['area'])
    ds = COCOKeypointEvalDataset(ld, n=1)
    assert len(ds) == 1 and ds[0][1].shape == (1, 17, 3)
    with pytest.raises(IndexError):
        ds[1]


def test_synthetic_keypoint_split():
    from chainer_maskrcnn.evaluator import SyntheticKeypointEvalDataset
    ds = SyntheticKeypointEvalDataset(3, 64, 80, G=4)
    img, kp, area, crowd, box = ds[1]
    assert img.shape == (3, 64, 80) and img.max() > 1.0 and kp.shape == (4, 17, 3) and (kp[:, :, 2] == 2).all()
    np.testing.assert_allclose(area, box[:, 2] * box[:, 3])
    assert not crowd.any()
    assert ((kp[:, :, 1] >= box[:, None, 0]) & (kp[:, :, 1] <= box[:, None, 0] + box[:, None, 2])).all()
    for x, y in zip(ds[1], SyntheticKeypointEvalDataset(3, 64, 80, G=4)[1]):
        np.testing.assert_array_equal(x, y)


def test_evaluator_needs_sigmas_for_other_keypoint_counts():
    from chainer_maskrcnn.evaluator import KeypointCOCOEvaluator

    class _T(object):
        class head(object):
            n_keypoints = 20
    with pytest.raises(ValueError, match='sigmas'):
        KeypointCOCOEvaluator([], _T())
    KeypointCOCOEvaluator([], _T(), sigmas=np.full(20, .05))


# ---- the C entry point's host checks -------------------------------------------------------------------------------------------------
def test_decode_argument_errors_are_reported_before_any_launch():
    from chainer_maskrcnn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_char * 4096)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)   # non-null, 16-byte aligned stand-ins: never dereferenced
    N = None
    ws = lib.mrcnn_keypoint_decode_workspace_bytes(3, 56, 17)
    assert ws > 0 and ws % (3 * 17 * 16) == 0
    assert lib.mrcnn_keypoint_decode_workspace_bytes(0, 56, 17) == 0 and lib.mrcnn_keypoint_decode_workspace_bytes(3, 56, 0) == 0

    def call(heat=P, D=3, S=56, Cp=32, K=17, bbox=P, w=P, wb=ws, out=P, idx=N):
        return lib.mrcnn_keypoint_decode_f32(heat, D, S, Cp, K, bbox, w, wb, out, idx, N)
    assert call(D=-1) == -1 and b'keypoint_decode' in lib.mrcnn_last_error()
    assert call(S=0) == -1 and call(K=0) == -1 and call(K=33) == -1
    assert call(Cp=18, K=17) == -1 and b'multiple of 4' in lib.mrcnn_last_error()
    assert call(K=257, Cp=260) == -2
    assert call(heat=N) == -1 and call(bbox=N) == -1 and call(out=N) == -1
    assert call(heat=ctypes.c_void_p(P.value + 4)) == -1 and b'aligned' in lib.mrcnn_last_error()
    assert call(out=ctypes.c_void_p(P.value + 8)) == -1
    assert call(wb=ws - 1) == -3 and b'workspace' in lib.mrcnn_last_error()
    assert call(w=N) == -3
    # D == 0: nothing to do, no pointer needed
    assert lib.mrcnn_keypoint_decode_f32(N, 0, 56, 32, 17, N, N, 0, N, N, N) == 0


def test_decode_op_has_no_cpu_fallback():
    import torch
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    with pytest.raises(_hip.MrcnnHipError):
        ops.keypoint_decode(torch.zeros(2, 56, 56, 32), torch.zeros(2, 4), 17)


# ---- train.py --eval-metric --------------------------------------------------------------------------------------------------------
def test_eval_metric_flag_and_refusals(monkeypatch):
    import train
    for kp in (False, True):
        p = train.build_parser(keypoints=kp)
        assert p.parse_args([]).eval_metric == 'mask_voc'
        assert p.parse_args(['--eval-metric', 'keypoint_coco']).eval_metric == 'keypoint_coco'
        with pytest.raises(SystemExit):
            p.parse_args(['--eval-metric', 'bbox'])
    kp_parser = train.build_parser(keypoints=True)
    with pytest.raises(ValueError, match='mask heads only') as e:                    # the default metric on a keypoint run
        train.run(kp_parser.parse_args(['--eval-interval', '5']), keypoints=True)
    assert 'keypoint_coco' in str(e.value)
    with pytest.raises(ValueError, match='keypoint head'):                           # the keypoint metric on a mask run
        train.run(train.build_parser().parse_args(['--eval-interval', '5', '--eval-metric', 'keypoint_coco']))
    with pytest.raises(ValueError, match='sigmas'):                                  # depth: 20 keypoints, no COCO sigmas
        train.run(kp_parser.parse_args(['--eval-interval', '5', '--eval-metric', 'keypoint_coco', '--dataset', 'depth']), keypoints=True)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='multi-GPU'):
        train.run(kp_parser.parse_args(['--eval-interval', '5', '--eval-metric', 'keypoint_coco']), keypoints=True)
