"""COCO box and mask AP on the host (chainer_maskrcnn/evaluations.py COCO part, dataset/coco_api.py rle_to_string, evaluator.py,
train.py --eval-metric mask_coco, evaluate.py) without a device:

* rle_to_string against rle_from_string, and one string worked out by hand;
* a literal restatement of pycocotools' COCOeval for iouType 'segm' / 'bbox' (maskApi.c's rleIou / bbIou pair by pair, computeIoU,
  evaluateImg, accumulate, summarize over dicts, as written there) against the streaming COCOInstanceMatchAccumulator on random
  multi-category data, and hand-worked cases;
* evaluate_coco_results on a small hand-written annotation file (polygon, uncompressed and compressed RLE);
* COCOMaskLoader.get_annotations and COCOInstanceEvalDataset on that file;
* the host argument checks of the three mrcnn_mask_rle_* entries through ctypes (nothing is launched);
* the refusals and flags of train.py --eval-metric mask_coco and evaluate.py."""
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
from chainer_maskrcnn.dataset import coco_api  # noqa: E402

ONE = pytest.approx(1.0, abs=1e-12)        # precision tp / (fp + tp + eps): a perfect score is 1 - 2e-16
STATS = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')


# ---- rle_to_string ---------------------------------------------------------------------------------------------------------------------
def test_rle_string_by_hand():
    # [0, 3, 1, 4]: '0', '3', '1', then 4 - 3 = 1 -> '1'.  [40]: 40 = 0b01000 + 1 << 5: groups 8 (| 0x20 = 40) then 1 -> 'X1'.
    assert coco_api.rle_to_string([0, 3, 1, 4]) == '0311'
    assert coco_api.rle_to_string([40]) == 'X1'
    assert coco_api.rle_to_string([5, 2, 3, 1]) == '523O'           # 1 - 2 = -1: one group 0x1f (sign bit set, nothing left): 'O'
    np.testing.assert_array_equal(coco_api.rle_from_string('X1'), [40])


@pytest.mark.parametrize('seed', range(5))
def test_rle_string_round_trip(seed):
    rs = np.random.RandomState(seed)
    cases = [[0], [7], [0, 5], [1 << 21], [0, 1 << 22, 3, (1 << 20) + 5, 1]]
    for _ in range(60):
        n = rs.randint(1, 40)
        c = rs.randint(0, 1 << rs.randint(1, 24), n)
        if rs.rand() < 0.5:
            c[0] = 0                                            # a first run of 0
        if n > 4 and rs.rand() < 0.5:
            c[4] = 0                                            # a delta far below the count two places before
        cases.append(c.tolist())
    for c in cases:
        s = coco_api.rle_to_string(c)
        assert all(48 <= ord(ch) < 48 + 64 for ch in s)
        np.testing.assert_array_equal(coco_api.rle_from_string(s), c)
    assert any(c[i] < c[i - 2] for c in cases for i in range(3, len(c)))          # negative deltas were exercised


def test_rle_strings_of_packed_runs_equal_one_by_one():
    rs = np.random.RandomState(9)
    runs = [rs.randint(0, 1 << rs.randint(1, 31), rs.randint(1, 30)).tolist() for _ in range(12)] + [[0], [3, 1 << 30, 0, 1]]
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in runs])))
    assert coco_api.rle_to_strings(offsets, np.concatenate(runs)) == [coco_api.rle_to_string(r) for r in runs]
    assert coco_api.rle_to_strings([0], []) == []


def test_rle_encode_restates_maskapi():
    m = np.zeros((3, 4), np.uint8)
    np.testing.assert_array_equal(coco_api.rle_encode(m), [12])
    m[0, 0] = 1
    np.testing.assert_array_equal(coco_api.rle_encode(m), [0, 1, 11])
    m[2, 3] = 7
    np.testing.assert_array_equal(coco_api.rle_encode(m), [0, 1, 10, 1])
    rs = np.random.RandomState(0)
    r = rs.rand(9, 11) < 0.4
    np.testing.assert_array_equal(coco_api.rle_decode(coco_api.rle_encode(r), 9, 11), r)


# ---- restatement of pycocotools (maskApi.c rleIou / bbIou, cocoeval.py COCOeval for 'segm' / 'bbox') --------------------------------
def _ref_iou(dts, gts, iou_type):
    o = np.zeros((len(dts), len(gts)))
    for g, gt in enumerate(gts):
        crowd = bool(gt['iscrowd'])
        for d, dt in enumerate(dts):
            if iou_type == 'segm':
                dm, gm = dt['mask'] != 0, gt['mask'] != 0
                i = int(np.count_nonzero(dm & gm))
                u = int(np.count_nonzero(dm)) if crowd else int(np.count_nonzero(dm)) + int(np.count_nonzero(gm)) - i
                o[d, g] = 0 if i == 0 else float(i) / float(u)
            else:
                D, G = dt['bbox'], gt['bbox']
                da, ga = D[2] * D[3], G[2] * G[3]
                w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
                if w <= 0:
                    continue
                h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
                if h <= 0:
                    continue
                i = w * h
                u = da if crowd else da + ga - i
                o[d, g] = i / u
    return o


def _ref_compute_iou(gt, dt, iou_type, max_det):
    if len(gt) == 0 and len(dt) == 0:
        return []
    inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
    dt = [dt[i] for i in inds]
    if len(dt) > max_det:
        dt = dt[0:max_det]
    if len(gt) == 0 or len(dt) == 0:
        return []
    return _ref_iou(dt, gt, iou_type)


def _ref_evaluate_img(gt, dt, ious, a_rng, max_det, iou_thrs):
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        if g['ignore'] or (g['area'] < a_rng[0] or g['area'] > a_rng[1]):
            g['_ignore'] = 1
        else:
            g['_ignore'] = 0
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


def _ref_accumulate(eval_imgs, n_cat, n_area, n_img, max_dets, iou_thrs, rec_thrs):
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), n_cat, n_area, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        Nk = k * A * n_img
        for a in range(A):
            Na = a * n_img
            for m, maxDet in enumerate(max_dets):
                E = [eval_imgs[Nk + Na + i] for i in range(n_img)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind='mergesort')
                dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
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
                    if nd:
                        recall[t, k, a, m] = rc[-1]
                    else:
                        recall[t, k, a, m] = 0
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
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def _ref_summarize(precision, recall, iou_thrs, max_dets):
    area_lbl = ['all', 'small', 'medium', 'large']

    def s(ap=1, iouThr=None, areaRng='all', maxDets=100):
        aind = [i for i, aRng in enumerate(area_lbl) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(max_dets) if mDet == maxDets]
        if ap == 1:
            x = precision
            if iouThr is not None:
                x = x[np.where(np.isclose(iouThr, iou_thrs))[0]]
            x = x[:, :, :, aind, mind]
        else:
            x = recall
            if iouThr is not None:
                x = x[np.where(np.isclose(iouThr, iou_thrs))[0]]
            x = x[:, :, aind, mind]
        return -1.0 if len(x[x > -1]) == 0 else float(np.mean(x[x > -1]))
    vals = (s(1), s(1, iouThr=.5), s(1, iouThr=.75), s(1, areaRng='small'), s(1, areaRng='medium'), s(1, areaRng='large'),
            s(0, maxDets=max_dets[0]), s(0, maxDets=max_dets[1]), s(0, maxDets=max_dets[2]), s(0, areaRng='small'),
            s(0, areaRng='medium'), s(0, areaRng='large'))
    return dict(zip(STATS, vals))


def ref_cocoeval(images, iou_type):
    """COCOeval over images = [(gts, dts)]: gts [{'category_id', 'area', 'iscrowd', 'mask' / 'bbox'}], dts [{'category_id', 'score',
    'area', 'mask' / 'bbox'}] (loadRes's area already set).  Ids and _prepare's ignore flag are added here; catIds = the sorted
    categories seen."""
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    max_dets = [1, 10, 100]
    a_rngs = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    cats = sorted({o['category_id'] for gts, dts in images for o in gts + dts})
    gid = did = 0
    G, Dd = {}, {}
    for i, (gts, dts) in enumerate(images):
        for g in gts:
            gid += 1
            g = dict(g, id=gid, ignore=int(bool(g['iscrowd'])))
            G.setdefault((i, g['category_id']), []).append(g)
        for d in dts:
            did += 1
            Dd.setdefault((i, d['category_id']), []).append(dict(d, id=did))
    ious = {(i, c): _ref_compute_iou(G.get((i, c), []), Dd.get((i, c), []), iou_type, max_dets[-1]) for i in range(len(images)) for c in cats}
    eval_imgs = [_ref_evaluate_img([dict(g) for g in G.get((i, c), [])], Dd.get((i, c), []), ious[i, c], a, max_dets[-1], iou_thrs)
                 for c in cats for a in a_rngs for i in range(len(images))]
    precision, recall = _ref_accumulate(eval_imgs, len(cats), len(a_rngs), len(images), max_dets, iou_thrs, rec_thrs)
    return _ref_summarize(precision, recall, iou_thrs, max_dets)


def accumulate(images, iou_type):
    """The same images through COCOInstanceMatchAccumulator, IoU from evaluations' vectorised rules (segm: exact counts)."""
    acc = evaluations.COCOInstanceMatchAccumulator()
    for gts, dts in images:
        crowd = np.array([bool(g['iscrowd']) for g in gts], bool)
        if iou_type == 'segm':
            dm = np.array([d['mask'] != 0 for d in dts]).reshape(len(dts), H * W).astype(np.int64)
            gm = np.array([g['mask'] != 0 for g in gts]).reshape(len(gts), H * W).astype(np.int64)
            iou = evaluations.segm_iou_from_counts(dm @ gm.T, dm.sum(1), gm.sum(1), crowd)
        else:
            iou = evaluations.bbox_iou_xywh([d['bbox'] for d in dts], [g['bbox'] for g in gts], crowd)
        acc.add_image(iou, [d['category_id'] for d in dts], [d['score'] for d in dts], [d['area'] for d in dts],
                      [g['category_id'] for g in gts], [g['area'] for g in gts], crowd)
    return acc.summarize()


def _both(images, iou_type):
    got = accumulate(images, iou_type)
    want = ref_cocoeval(images, iou_type)
    assert got == want, (iou_type, got, want)
    return got


# ---- random cases ------------------------------------------------------------------------------------------------------------------------
H, W = 36, 40                                   # 1440 pixels: masks reach every area range of the segm detections


def _rect_mask(rs):
    m = np.zeros((H, W), np.uint8)
    y0, x0 = rs.randint(0, H), rs.randint(0, W)
    m[y0:y0 + rs.randint(1, H + 1), x0:x0 + rs.randint(1, W + 1)] = 1
    return m


def _random_images(rs, iou_type, n_img, n_cat=4):
    images = []
    for i in range(n_img):
        gts, dts = [], []
        for _ in range(rs.randint(0, 6) if i % 4 else 0):                 # every fourth image: no ground truth
            m = _rect_mask(rs)
            ys, xs = np.nonzero(m)
            box = [float(xs.min()) + rs.rand(), float(ys.min()) + rs.rand(), float(np.ptp(xs) + 1) * rs.uniform(.5, 30),
                   float(np.ptp(ys) + 1) * rs.uniform(.5, 30)]
            area = rs.choice([float(m.sum()) * rs.uniform(.2, 60), 32. ** 2, 96. ** 2, rs.uniform(0, 20000)])
            gts.append({'category_id': int(rs.randint(1, n_cat + 1)) * 3, 'area': float(area), 'iscrowd': int(rs.rand() < 0.15),
                        'mask': m, 'bbox': box})
        n_dt = 0 if i % 5 == 2 else rs.randint(0, 25)                    # some images without detections
        if i == 1:
            n_dt = 130                                                    # more than 100 in one category of one image
        for j in range(n_dt):
            if gts and rs.rand() < 0.7:
                g = gts[rs.randint(len(gts))]
                m = g['mask'].copy()
                if rs.rand() < 0.5:
                    m = np.roll(m, rs.randint(-3, 4), axis=rs.randint(2))
                box = [v + rs.standard_normal() * rs.choice([0.0, .5, 3.0]) for v in g['bbox']]
                cat = g['category_id'] if rs.rand() < 0.85 else int(rs.randint(1, n_cat + 1)) * 3
            else:
                m = _rect_mask(rs) if rs.rand() < 0.9 else np.zeros((H, W), np.uint8)     # some empty masks
                box = [rs.uniform(0, 40), rs.uniform(0, 40), rs.uniform(1, 200), rs.uniform(1, 200)]
                cat = int(rs.randint(1, n_cat + 1)) * 3
            if i == 1:
                cat = 6
            box[2], box[3] = abs(box[2]) + 0.25, abs(box[3]) + 0.25
            area = float(np.count_nonzero(m)) if iou_type == 'segm' else box[2] * box[3]
            dts.append({'category_id': cat, 'score': float(np.round(rs.rand(), 1)), 'area': area, 'mask': m, 'bbox': box})
        images.append((gts, dts))
    return images


@pytest.mark.parametrize('iou_type', ['segm', 'bbox'])
@pytest.mark.parametrize('seed', range(4))
def test_streaming_accumulator_equals_the_restatement_on_random_data(iou_type, seed):
    rs = np.random.RandomState(200 + seed)
    images = _random_images(rs, iou_type, rs.randint(5, 11))
    got = _both(images, iou_type)
    assert any(v > 0 for v in got.values())


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------------------
def _gt(m, cat=1, crowd=0, area=None, box=None):
    ys, xs = np.nonzero(m) if m.any() else (np.zeros(1), np.zeros(1))
    box = box or [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
    return {'category_id': cat, 'area': float(m.sum()) if area is None else area, 'iscrowd': crowd, 'mask': m, 'bbox': box}


def _dt(g, score, iou_type='segm', **kw):
    d = {'category_id': g['category_id'], 'score': score, 'mask': g['mask'], 'bbox': list(g['bbox'])}
    d.update(kw)
    d['area'] = float(np.count_nonzero(d['mask'])) if iou_type == 'segm' else d['bbox'][2] * d['bbox'][3]
    return d


def _blob(y0, x0, h, w):
    m = np.zeros((H, W), np.uint8)
    m[y0:y0 + h, x0:x0 + w] = 1
    return m


@pytest.mark.parametrize('iou_type', ['segm', 'bbox'])
def test_ground_truth_as_detections_scores_one(iou_type):
    imgs = [[_gt(_blob(0, 0, 5, 6), 1), _gt(_blob(10, 10, 20, 25), 2, area=2000.), _gt(_blob(20, 0, 3, 3), 1, area=9500.)],
            [_gt(_blob(2, 3, 30, 30), 2, area=500.)]]
    images = [(g, [_dt(x, 0.9 - 0.1 * j, iou_type) for j, x in enumerate(g)]) for g in imgs]
    r = _both(images, iou_type)
    for k, v in r.items():
        assert v == -1.0 or v == ONE or k == 'AR1', (k, v)
    assert r['AP'] == ONE and r['APm'] == ONE and r['APl'] == ONE
    assert r['AR1'] == 0.75                        # one detection per image: category 1 finds 1 of its 2, category 2 both of its


def test_no_detections():
    assert _both([([], []), ([], [])], 'segm') == dict.fromkeys(STATS, -1.0)                 # nothing at all: every stat -1
    r = _both([([_gt(_blob(0, 0, 5, 5))], [])], 'segm')                                       # ground truth only: precision 0
    assert r['AP'] == 0.0 and r['AR100'] == 0.0 and r['APm'] == -1.0


@pytest.mark.parametrize('iou_type', ['segm', 'bbox'])
def test_crowd_absorbs_two_detections(iou_type):
    g = _gt(_blob(0, 0, 10, 10), 1)
    crowd = _gt(_blob(15, 15, 20, 20), 1, crowd=1)
    d_tp = _dt(g, 0.5, iou_type)
    d_c1, d_c2 = _dt(crowd, 0.9, iou_type), _dt(crowd, 0.8, iou_type, mask=_blob(15, 15, 10, 10), bbox=[15., 15., 10., 10.])
    r = _both([([g, crowd], [d_c1, d_c2, d_tp])], iou_type)
    assert r['AP'] == ONE and r['AR100'] == 1.0                     # both on the crowd are ignored, not false positives
    crowd0 = dict(crowd, iscrowd=0)
    r2 = _both([([g, crowd0], [d_c1, d_c2, d_tp])], iou_type)
    # without the crowd flag the second is a false positive at IoU .25 (inside the crowd's box): hit, miss, hit over two ground
    # truths -> precision 1 up to recall .5, 2/3 above
    assert r2['AR100'] == 1.0 and r2['AP50'] == pytest.approx((51 + 50 * 2 / 3) / 101, abs=1e-12)


def test_empty_mask_has_iou_zero():
    iou = evaluations.segm_iou_from_counts(np.zeros((2, 2)), [0, 5], [0, 7], [False, True])
    assert iou.dtype == np.float64 and (iou == 0).all() and not np.isnan(iou).any()
    np.testing.assert_array_equal(evaluations.segm_iou_from_counts([[3, 3]], [4], [6, 8], [False, True]), [[3 / 7, 3 / 4]])
    g = _gt(_blob(0, 0, 4, 4))
    empty = _dt(g, 0.9, mask=np.zeros((H, W), np.uint8))
    r = _both([([g], [empty, _dt(g, 0.5)])], 'segm')
    # the empty mask is a false positive ranked first: precision 0 then 1/2 -> envelope 1/2 everywhere
    assert r['AP'] == pytest.approx(0.5, abs=1e-12)


def test_box_iou_by_hand():
    iou = evaluations.bbox_iou_xywh([[0, 0, 10, 10], [5, 5, 10, 10], [20, 20, 1, 1]], [[0, 0, 10, 10], [5, 0, 10, 10]], [False, True])
    np.testing.assert_allclose(iou, [[1, 50 / 100], [25 / 175, 50 / 100], [0, 0]], rtol=1e-15)


def test_area_range_edges_are_closed():
    g1, g2 = _gt(_blob(0, 0, 32, 32), 1, area=32. ** 2), _gt(_blob(0, 0, 5, 5), 2, area=96. ** 2)
    images = [([g1, g2], [_dt(g1, .9), _dt(g2, .8)])]
    r = _both(images, 'segm')
    assert r['APs'] == ONE and r['APm'] == ONE and r['APl'] == ONE       # 32^2 is small and medium, 96^2 medium and large


# ---- evaluate_coco_results on a hand-written annotation file -------------------------------------------------------------------------
def _gt_file(tmp_path):
    # 10 x 12 image 1: a polygon square (cat 1), an uncompressed RLE (cat 2), a compressed-RLE crowd (cat 2); image 2: no annotation
    h, w = 10, 12
    rle2 = np.zeros((h, w), np.uint8)
    rle2[6:9, 1:4] = 1
    crowd = np.zeros((h, w), np.uint8)
    crowd[0:4, 8:12] = 1
    anno = {'images': [{'id': 1, 'file_name': 'a.png', 'height': h, 'width': w}, {'id': 2, 'file_name': 'b.png', 'height': h, 'width': w}],
            'categories': [{'id': 1, 'name': 'one'}, {'id': 2, 'name': 'two'}, {'id': 5, 'name': 'five'}],
            'annotations': [
                {'id': 10, 'image_id': 1, 'category_id': 1, 'segmentation': [[1, 1, 5, 1, 5, 5, 1, 5]], 'area': 16.0, 'iscrowd': 0,
                 'bbox': [1, 1, 4, 4]},
                {'id': 11, 'image_id': 1, 'category_id': 2, 'segmentation': {'counts': coco_api.rle_encode(rle2).tolist(), 'size': [h, w]},
                 'area': 9.0, 'iscrowd': 0, 'bbox': [1, 6, 3, 3]},
                {'id': 12, 'image_id': 1, 'category_id': 2, 'segmentation': {'counts': coco_api.rle_to_string(coco_api.rle_encode(crowd)),
                                                                              'size': [h, w]}, 'area': 16.0, 'iscrowd': 1, 'bbox': [8, 0, 4, 4]}]}
    p = tmp_path / 'instances_val2017.json'
    p.write_text(json.dumps(anno))
    c = coco_api.COCO(str(p))
    masks = {a['id']: c.annToMask(a) for a in anno['annotations']}
    return str(p), masks


def _seg(m):
    return {'size': list(m.shape), 'counts': coco_api.rle_to_string(coco_api.rle_encode(m))}


def test_evaluate_coco_results_by_hand(tmp_path):
    path, masks = _gt_file(tmp_path)
    assert masks[10].sum() == 16 and masks[11].sum() == 9 and masks[12].sum() == 16
    miss = np.zeros((10, 12), np.uint8)
    miss[8:10, 8:12] = 1                                            # overlaps nothing
    segm = [{'image_id': 1, 'category_id': 1, 'segmentation': _seg(masks[10]), 'score': 0.9},
            {'image_id': 1, 'category_id': 2, 'segmentation': _seg(masks[12]), 'score': 0.99},     # on the crowd: ignored
            {'image_id': 1, 'category_id': 2, 'segmentation': _seg(miss), 'score': 0.95},          # false positive, ranked first
            {'image_id': 1, 'category_id': 2, 'segmentation': _seg(masks[11]), 'score': 0.8},
            {'image_id': 2, 'category_id': 1, 'segmentation': _seg(masks[10]), 'score': 0.1},      # an image without ground truth
            {'image_id': 1, 'category_id': 7, 'segmentation': _seg(masks[10]), 'score': 0.5}]      # not a category of the file
    r = evaluations.evaluate_coco_results(path, segm, 'segm')
    # cat 1: hit (0.9) then a false positive (0.1, image 2): precision 1 up to recall 1 -> AP 1.  cat 2: miss then hit -> 1/2.
    assert r['AP'] == pytest.approx(0.75, abs=1e-12) and r['AP50'] == r['AP75'] == r['AP'] == r['APs']
    assert r['APm'] == -1.0 and r['APl'] == -1.0
    assert r['AR1'] == pytest.approx(0.5) and r['AR10'] == 1.0 and r['AR100'] == 1.0 and r['ARs'] == 1.0
    f = tmp_path / 'segm.json'
    f.write_text(json.dumps(segm))
    assert evaluations.evaluate_coco_results(path, str(f), 'segm') == r                 # a results file reads the same
    assert evaluations.evaluate_coco_results(path, segm, 'segm', img_ids=[1])['AP'] == pytest.approx(0.75, abs=1e-12)
    box = lambda m: [float(np.nonzero(m)[1].min()), float(np.nonzero(m)[0].min()), float(np.ptp(np.nonzero(m)[1]) + 1),
                     float(np.ptp(np.nonzero(m)[0]) + 1)]
    bbox = [{k: v for k, v in d.items() if k != 'segmentation'} for d in segm]
    for d, m in zip(bbox, (masks[10], masks[12], miss, masks[11], masks[10], masks[10])):
        d['bbox'] = box(m)
    rb = evaluations.evaluate_coco_results(path, bbox, 'bbox')
    assert rb == r                                                  # the boxes of the masks give the same matches here
    with pytest.raises(ValueError):
        evaluations.evaluate_coco_results(path, bbox, 'keypoints')


def test_coco_instance_eval_dataset_and_mask_loader_annotations(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOInstanceEvalDataset, COCOMaskLoader
    _gt_file(tmp_path)
    ld = COCOMaskLoader(anno_dir=str(tmp_path), img_dir=str(tmp_path / 'none'), split='val', data_type='2017')
    assert len(ld) == 1                                              # image 2 has no annotation
    a = ld.get_annotations(0)
    np.testing.assert_array_equal(a['area'], [16., 9., 16.])
    np.testing.assert_array_equal(a['iscrowd'], [False, False, True])
    np.testing.assert_array_equal(a['category_id'], [1, 2, 2])
    np.testing.assert_array_equal(a['bbox'], [[1, 1, 4, 4], [1, 6, 3, 3], [8, 0, 4, 4]])
    assert a['image_id'] == 1 and a['bbox'].dtype == np.float64
    ds = COCOInstanceEvalDataset(anno_dir=str(tmp_path), img_dir=str(tmp_path / 'none'))
    assert len(ds) == 2 and ds.img_ids == [1, 2] and ds.cat_ids == [1, 2, 5] and ds.label_names == ['one', 'two', 'five']
    assert ds.get_annotations(1)['area'].shape == (0,) and ds.get_annotations(1)['image_id'] == 2
    assert len(COCOInstanceEvalDataset(anno_dir=str(tmp_path), img_dir='none', n=1)) == 1
    f = COCOInstanceEvalDataset(anno_dir=str(tmp_path), img_dir='none', category_filter=['two'])
    assert f.cat_ids == [2] and list(f.get_annotations(0)['category_id']) == [2, 2]
    with pytest.raises(IndexError):
        ds.get_annotations(2)


def test_synthetic_coco_split():
    from chainer_maskrcnn.evaluator import SyntheticCOCOEvalDataset
    ds = SyntheticCOCOEvalDataset(3, 64, 80, n_fg_class=10, G=4)
    img, m, lab, area, crowd, box, img_id = ds[2]
    assert img.shape == (3, 64, 80) and m.shape == (4, 64, 80) and img_id == 2 and not crowd.any()
    np.testing.assert_array_equal(area, (m != 0).reshape(4, -1).sum(1))
    assert box.shape == (4, 4) and (box[:, 2:] > 0).all() and ds.cat_ids == list(range(10))


def test_split_results_and_summary_lines():
    from chainer_maskrcnn.evaluator import split_coco_results
    r = [{'image_id': 1, 'category_id': 2, 'segmentation': {'size': [2, 2], 'counts': '04'}, 'bbox': [0., 0., 1., 1.], 'score': .5}]
    s, b = split_coco_results(r)
    assert 'bbox' not in s[0] and 'segmentation' not in b[0] and s[0]['score'] == b[0]['score'] == .5
    txt = evaluations.format_coco_stats(dict(zip(STATS, np.linspace(0, 1, 12))), 'segm')
    lines = txt.split('\n')
    assert len(lines) == 13 and lines[1] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.000'
    assert lines[7].startswith(' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ]')


# ---- the C entry points' host checks ---------------------------------------------------------------------------------------------------
def test_rle_argument_errors_are_reported_before_any_launch():
    from chainer_maskrcnn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_char * 4096)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)   # non-null stand-ins: never dereferenced
    N = None
    ws = lib.mrcnn_mask_rle_workspace_bytes(3, 100, 70)
    assert ws >= 3 * 70 * 2 * 8 and lib.mrcnn_mask_rle_workspace_bytes(-1, 5, 5) == 0
    assert lib.mrcnn_mask_rle_workspace_bytes(3, 0, 70) < ws

    def count(m=P, D=3, H=100, W=70, w=P, wb=ws, off=P, area=N):
        return lib.mrcnn_mask_rle_count_u8(m, D, H, W, w, wb, off, area, N)

    def write(m=P, D=3, H=100, W=70, w=P, wb=ws, off=P, cnt=P):
        return lib.mrcnn_mask_rle_write_u8(m, D, H, W, w, wb, off, cnt, N)
    for f in (count, write):
        assert f(D=-1) == -1 and b'negative' in lib.mrcnn_last_error()
        assert f(H=-2) == -1 and f(W=-3) == -1
        assert f(m=N) == -1 and b'null' in lib.mrcnn_last_error()
        assert f(off=N) == -1
        assert f(wb=ws - 1) == -3 and b'workspace' in lib.mrcnn_last_error()
        assert f(w=N) == -3
        assert f(H=50000, W=50000) == -2 and b'int32' in lib.mrcnn_last_error()          # H * W > 2^31 - 1
        assert f(D=3000, H=1000, W=1000) == -2                                            # the worst-case run total
    assert write(cnt=N) == -1
    assert lib.mrcnn_mask_rle_write_u8(N, 0, 5, 5, N, 0, N, N, N) == 0                   # D == 0: nothing to write


def test_rle_op_has_no_cpu_fallback():
    import torch
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    with pytest.raises(_hip.MrcnnHipError):
        ops.mask_rle_encode(torch.zeros(2, 5, 6, dtype=torch.bool))


# ---- train.py --eval-metric mask_coco and evaluate.py ---------------------------------------------------------------------------------
def test_train_mask_coco_flag_and_refusals(monkeypatch):
    import train
    for kp in (False, True):
        assert train.build_parser(keypoints=kp).parse_args(['--eval-metric', 'mask_coco']).eval_metric == 'mask_coco'
        assert train.build_parser(keypoints=kp).parse_args([]).eval_metric == 'mask_voc'
    kp_parser = train.build_parser(keypoints=True)
    with pytest.raises(ValueError, match='mask heads only') as e:                    # a keypoint run cannot take mask_coco
        train.run(kp_parser.parse_args(['--eval-interval', '5', '--eval-metric', 'mask_coco']), keypoints=True)
    assert 'mask_coco' in str(e.value) and 'keypoint_coco' in str(e.value)
    with pytest.raises(ValueError, match='mask_coco'):                               # the keypoint metric on a mask run names both
        train.run(train.build_parser().parse_args(['--eval-interval', '5', '--eval-metric', 'keypoint_coco']))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='single-process'):
        train.run(train.build_parser().parse_args(['--eval-interval', '5', '--eval-metric', 'mask_coco']))


def test_evaluate_flags_and_refusals(monkeypatch):
    import evaluate
    a = evaluate.build_parser().parse_args([])
    assert (a.split, a.synthetic, a.eval_images, a.score_thresh, a.no_results, a.head_arch) == ('val', 0, 0, None, False, 'fpn')
    a = evaluate.build_parser().parse_args(['--weight', 'm.npz', '--score-thresh', '0.01', '--no-results', '--synthetic', '1',
                                            '--image-size', '64', '80', '--eval-images', '3', '--out', 'o', '--label_file', 'l.txt',
                                            '--backbone', 'fpn', '--anno-dir', 'a', '--img-dir', 'i', '--data-type', '2014'])
    assert (a.weight, a.score_thresh, a.no_results, a.image_size, a.eval_images, a.out) == ('m.npz', 0.01, True, [64, 80], 3, 'o')
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(['--split', 'test'])
    with pytest.raises(ValueError, match='train_keypoints.py --eval-metric keypoint_coco'):
        evaluate.run(evaluate.build_parser().parse_args(['--head-arch', 'fpn_keypoint']))
    monkeypatch.setenv('WORLD_SIZE', '4')
    with pytest.raises(ValueError, match='single process'):
        evaluate.run(evaluate.build_parser().parse_args([]))
