"""Boundary AP on the host (no device): the band-width rule at its pinned values, evaluations.mask_boundary against the literal restatement
(boundary_reference.py), the pair rule on hand-worked pairs, the streaming accumulator fed Boundary IoUs against the restated COCOeval of
test_coco_eval_cpu.py fed the same IoUs, the host argument checks of the three new C entry points through ctypes (nothing is launched),
and the flags of evaluate.py / train.py / train_keypoints.py."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'chainer-maskrcnn_amd'), ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import boundary_reference as bref  # noqa: E402
import test_coco_eval_cpu as tcc  # noqa: E402
from chainer_maskrcnn import evaluations  # noqa: E402


# ---- the band width -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw,d', sorted(bref.PINNED_DILATIONS.items()))
def test_pinned_dilations(hw, d):
    assert evaluations.boundary_dilation(*hw) == d == bref.ref_dilation(*hw)
    assert isinstance(evaluations.boundary_dilation(*hw), int)


def test_dilation_rounds_half_to_even_and_is_at_least_one():
    assert 0.02 * np.sqrt(375.0 ** 2 + 500.0 ** 2) == 12.5 and evaluations.boundary_dilation(375, 500) == 12
    assert 0.02 * np.sqrt(75.0 ** 2 + 100.0 ** 2) == 2.5 and evaluations.boundary_dilation(75, 100) == 2
    assert evaluations.boundary_dilation(105, 140) == 4                        # 3.5 rounds up to the even 4
    assert evaluations.boundary_dilation(3, 4) == 1 and evaluations.boundary_dilation(0, 0) == 1
    assert evaluations.boundary_dilation(300, 400, ratio=0.01) == 5


# ---- the band ------------------------------------------------------------------------------------------------------------------------------
def _families(H, W, d, rs):
    out = []

    def new():
        out.append(np.zeros((H, W), np.uint8))
        return out[-1]
    new()[:] = 1
    new()
    new()[H // 2, W // 2] = 1
    hh, hw = max(H // 2, 1), max(W // 2, 1)
    new()[:hh, W // 4:W // 4 + hw] = 1
    new()[H - hh:, W // 4:W // 4 + hw] = 1
    new()[H // 4:H // 4 + hh, :hw] = 1
    new()[H // 4:H // 4 + hh, W - hw:] = 1
    m = new()
    m[1:H - 1, 1:W - 1] = 1
    m[H // 2, W // 2] = 0
    new()[:] = rs.rand(H, W) < 0.9
    new()[:] = (rs.rand(H, W) < 0.95) * np.where(rs.rand(H, W) < 0.5, 255, 2)
    return np.stack(out)


@pytest.mark.parametrize('H,W,d', [(1, 1, 1), (2, 63, 2), (37, 70, 3), (70, 129, 16), (40, 30, 33), (2, 1, 3), (64, 65, 31), (130, 131, 63),
                                   (16, 64, 16), (33, 200, 16), (75, 100, 2)])
def test_mask_boundary_equals_the_restatement(H, W, d):
    m = _families(H, W, d, np.random.RandomState(H + W + d))
    got = evaluations.mask_boundary(m, d)
    assert got.dtype == bool and got.shape == m.shape
    np.testing.assert_array_equal(got, bref.ref_boundaries(m, d))
    np.testing.assert_array_equal(evaluations.mask_boundary(m[3], d), got[3])            # a single (H, W) mask
    if d > H or d > W:
        np.testing.assert_array_equal(got, m != 0)
    if H > 2 * d and W > 2 * d:
        frame = np.ones((H, W), bool)
        frame[d:H - d, d:W - d] = False
        np.testing.assert_array_equal(got[0], frame)
    with pytest.raises(ValueError, match='dilation'):
        evaluations.mask_boundary(m, 0)


# ---- the pair rule, by hand --------------------------------------------------------------------------------------------------------------------
def _square(y0, x0, n, H=100, W=100):
    m = np.zeros((H, W), np.uint8)
    m[y0:y0 + n, x0:x0 + n] = 1
    return m


def _pair(dm, gm, d, crowd=False):
    """(mask IoU, band IoU, pair IoU) from the product's functions, counts taken with the product's mask_boundary."""
    db, gb = evaluations.mask_boundary(dm, d), evaluations.mask_boundary(gm, d)
    cnt = lambda x, y: np.array([[np.count_nonzero((x != 0) & (y != 0))]])
    area = lambda x: np.array([np.count_nonzero(x)])
    c = [crowd]
    mi = evaluations.segm_iou_from_counts(cnt(dm, gm), area(dm), area(gm), c)[0, 0]
    bi = evaluations.segm_iou_from_counts(cnt(db, gb), area(db), area(gb), c)[0, 0]
    pi = evaluations.boundary_iou_from_counts(cnt(dm, gm), area(dm), area(gm), cnt(db, gb), area(db), area(gb), c)
    assert pi.shape == (1, 1) and pi.dtype == np.float64
    assert (mi, bi, pi[0, 0]) == bref.ref_pair_iou(dm, gm, d, crowd)
    return mi, bi, pi[0, 0]


def test_pair_rule_by_hand():
    d = 3
    a = _square(30, 30, 40)
    # the band of a 40 x 40 square, d = 3: 40^2 - 34^2 = 444 pixels
    assert np.count_nonzero(evaluations.mask_boundary(a, d)) == 444
    assert _pair(a, a, d) == (1.0, 1.0, 1.0)
    # shifted by 2 px: the masks share 38 x 40 = 1520 of 3200 - 1520 = 1680; the bands share 1520 - (2 * 34^2 - 32 * 34) = 296 of
    # 888 - 296 = 592
    b = _square(30, 32, 40)
    assert _pair(b, a, d) == (float(Fraction(1520, 1680)), float(Fraction(296, 592)), 0.5)
    # a crowd ground truth: over the detection's own counts, 1520 / 1600 and 296 / 444
    assert _pair(b, a, d, crowd=True) == (1520 / 1600, 296 / 444, 296 / 444)
    # no common band pixel: a 10 x 10 square in the middle of the 40 x 40 one overlaps the mask, not its rim
    c = _square(45, 45, 10)
    assert _pair(c, a, d) == (100 / 1600, 0.0, 0.0)
    # no common pixel at all, and an empty mask
    assert _pair(_square(0, 0, 10), a, d) == (0.0, 0.0, 0.0)
    assert _pair(np.zeros_like(a), a, d) == (0.0, 0.0, 0.0)
    # the band IoU can also be the larger one: then the mask IoU is the pair's
    thin = np.zeros_like(a)
    thin[30:70, 30:33] = 1                          # the square's left rim: all of it is band of both
    mi, bi, pi = _pair(thin, a, d)
    assert (mi, bi, pi) == (120 / 1600, 120 / 444, 120 / 1600)


def test_boundary_iou_from_counts_shapes_and_crowd_columns():
    inter = np.array([[10, 0, 4], [0, 0, 6]])
    binter = np.array([[5, 0, 4], [0, 0, 1]])
    got = evaluations.boundary_iou_from_counts(inter, [20, 8], [10, 5, 40], binter, [10, 6], [8, 5, 12], [False, False, True])
    want = np.array([[min(10 / 20, 5 / 13), 0.0, min(4 / 20, 4 / 10)], [0.0, 0.0, min(6 / 8, 1 / 6)]])
    np.testing.assert_array_equal(got, want)
    assert evaluations.boundary_iou_from_counts(np.zeros((0, 2)), [], [3, 4], np.zeros((0, 2)), [], [2, 2], [0, 1]).shape == (0, 2)


# ---- the accumulator fed Boundary IoUs ------------------------------------------------------------------------------------------------------
def _accumulate_boundary(images):
    """images of test_coco_eval_cpu's form through COCOInstanceMatchAccumulator, IoU from the product's host functions."""
    acc = evaluations.COCOInstanceMatchAccumulator()
    H, W = tcc.H, tcc.W
    d = evaluations.boundary_dilation(H, W)
    for gts, dts in images:
        crowd = np.array([bool(g['iscrowd']) for g in gts], bool)
        dm = np.array([x['mask'] != 0 for x in dts]).reshape(len(dts), H, W)
        gm = np.array([x['mask'] != 0 for x in gts]).reshape(len(gts), H, W)
        db, gb = evaluations.mask_boundary(dm, d), evaluations.mask_boundary(gm, d)
        flat = lambda x: x.reshape(len(x), H * W).astype(np.int64)
        iou = evaluations.boundary_iou_from_counts(flat(dm) @ flat(gm).T, flat(dm).sum(1), flat(gm).sum(1), flat(db) @ flat(gb).T,
                                                   flat(db).sum(1), flat(gb).sum(1), crowd)
        acc.add_image(iou, [x['category_id'] for x in dts], [x['score'] for x in dts], [x['area'] for x in dts],
                      [g['category_id'] for g in gts], [g['area'] for g in gts], crowd)
    return acc.summarize()


def _ref_boundary_cocoeval(images, monkeypatch):
    with monkeypatch.context() as mp:
        mp.setattr(tcc, '_ref_iou', bref.ref_cocoeval_boundary_iou)
        return tcc.ref_cocoeval(images, 'segm')


@pytest.mark.parametrize('seed', range(4))
def test_streaming_accumulator_with_boundary_ious_equals_the_restatement(seed, monkeypatch):
    rs = np.random.RandomState(200 + seed)
    images = tcc._random_images(rs, 'segm', rs.randint(5, 11))
    got = _accumulate_boundary(images)
    want = _ref_boundary_cocoeval(images, monkeypatch)
    assert got == want, (got, want)
    assert any(v > 0 for v in got.values())
    segm = tcc.accumulate(images, 'segm')
    assert segm == tcc.ref_cocoeval(images, 'segm')                               # the stand-in IoU is gone again
    for k in tcc.STATS:
        if got[k] > -1 and segm[k] > -1:
            assert got[k] <= segm[k], (k, got[k], segm[k])


def test_ground_truth_as_detections_scores_boundary_ap_one(monkeypatch):
    imgs = [[tcc._gt(tcc._blob(0, 0, 5, 6), 1), tcc._gt(tcc._blob(10, 10, 20, 25), 2, area=2000.), tcc._gt(tcc._blob(20, 0, 3, 3), 1, area=9500.)],
            [tcc._gt(tcc._blob(2, 3, 30, 30), 2, area=500.)]]
    images = [(g, [tcc._dt(x, 0.9 - 0.1 * j) for j, x in enumerate(g)]) for g in imgs]
    got = _accumulate_boundary(images)
    assert got == _ref_boundary_cocoeval(images, monkeypatch)
    for k, v in got.items():
        assert v == -1.0 or v == tcc.ONE or k == 'AR1', (k, v)
    assert got['AP'] == tcc.ONE and got['AR100'] == tcc.ONE
    assert got['AR1'] == 0.75                      # one detection per image: category 1 finds 1 of its 2, category 2 both of its


def test_evaluate_coco_results_boundary(tmp_path, monkeypatch):
    """A segm results file scored on the host with 'boundary': the restated COCOeval on the same masks (d from each image's size)."""
    import json
    from chainer_maskrcnn.dataset import coco_api
    rs = np.random.RandomState(4)
    H, W = 60, 90                                                                       # d = round(0.02 * 108.2) = 2
    images, anns, results, ref_images = [], [], [], []
    for i in range(3):
        images.append({'id': i + 1, 'height': H, 'width': W, 'file_name': '%d.png' % i})
        gts, dts = [], []
        for j in range(3):
            m = np.zeros((H, W), np.uint8)
            y0, x0 = rs.randint(0, 30), rs.randint(0, 50)
            m[y0:y0 + rs.randint(8, 30), x0:x0 + rs.randint(8, 40)] = 1
            cat = int(rs.randint(1, 3))
            crowd = int(i == 1 and j == 0)
            seg = {'size': [H, W], 'counts': coco_api.rle_to_string(coco_api.rle_encode(m))}
            anns.append({'id': len(anns) + 1, 'image_id': i + 1, 'category_id': cat, 'iscrowd': crowd, 'area': float(m.sum()),
                         'bbox': [0., 0., 1., 1.], 'segmentation': seg})
            gts.append({'category_id': cat, 'area': float(m.sum()), 'iscrowd': crowd, 'mask': m})
            p = np.roll(m, (j, i), axis=(0, 1))
            score = float(np.round(0.9 - 0.1 * j - 0.01 * i, 3))
            results.append({'image_id': i + 1, 'category_id': cat, 'score': score,
                            'segmentation': {'size': [H, W], 'counts': coco_api.rle_to_string(coco_api.rle_encode(p))}})
            dts.append({'category_id': cat, 'score': score, 'area': float(p.sum()), 'mask': p})
        ref_images.append((gts, dts))
    ann_file = tmp_path / 'instances.json'
    ann_file.write_text(json.dumps({'images': images, 'annotations': anns, 'categories': [{'id': 1, 'name': 'a'}, {'id': 2, 'name': 'b'}]}))
    assert evaluations.boundary_dilation(H, W) == 2
    got = evaluations.evaluate_coco_results(str(ann_file), results, 'boundary')
    assert got == _ref_boundary_cocoeval(ref_images, monkeypatch)
    segm = evaluations.evaluate_coco_results(str(ann_file), results, 'segm')
    assert segm == tcc.ref_cocoeval(ref_images, 'segm') and 0 < got['AP'] < segm['AP']
    with pytest.raises(ValueError, match="'boundary'"):
        evaluations.evaluate_coco_results(str(ann_file), results, 'keypoints')


def test_format_coco_stats_boundary():
    txt = evaluations.format_coco_stats(dict(zip(tcc.STATS, np.linspace(0, 1, 12))), 'boundary')
    lines = txt.split('\n')
    assert len(lines) == 13 and lines[0] == 'iouType: boundary'
    assert lines[1] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.000'
    assert lines[12] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 1.000'


def test_evaluator_accepts_boundary_and_refuses_other_types():
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator
    assert InstanceSegmentationCOCOEvaluator([], None).iou_types == ('segm', 'bbox')
    ev = InstanceSegmentationCOCOEvaluator([], None, iou_types=('segm', 'bbox', 'boundary'))
    assert set(ev._accumulator()) == {'segm', 'bbox', 'boundary'}
    assert InstanceSegmentationCOCOEvaluator([], None, iou_types=('boundary',)).iou_types == ('boundary',)
    for bad in ((), ('segm', 'keypoints'), ('Boundary',)):
        with pytest.raises(ValueError, match='boundary'):
            InstanceSegmentationCOCOEvaluator([], None, iou_types=bad)


# ---- the C entry points' host checks (no launch) ---------------------------------------------------------------------------------------------
def _lib():
    from chainer_maskrcnn import _hip
    return _hip.lib()


def test_symbols_are_declared():
    from chainer_maskrcnn import _hip
    for name in ('mrcnn_mask_boundary_workspace_bytes', 'mrcnn_mask_boundary_words_u8', 'mrcnn_mask_boundary_iou_counts_u8'):
        assert name in _hip.SIGNATURES and hasattr(_lib(), name)
    assert _hip.ABI_VERSION == 10


def test_boundary_workspace_query():
    lib = _lib()
    assert lib.mrcnn_mask_boundary_workspace_bytes(100, 20, 375, 500) == 2 * 120 * 375 * 8 * 8
    assert lib.mrcnn_mask_boundary_workspace_bytes(100, 20, 1024, 1024) == 2 * 120 * 1024 * 16 * 8
    assert lib.mrcnn_mask_boundary_workspace_bytes(1, 1, 1, 1) == 32
    assert lib.mrcnn_mask_boundary_workspace_bytes(3, 0, 10, 65) == 2 * 3 * 10 * 2 * 8
    assert lib.mrcnn_mask_boundary_workspace_bytes(0, 0, 1024, 1024) == 0 and lib.mrcnn_mask_boundary_workspace_bytes(5, 5, 0, 64) == 0
    for bad in ((-1, 2, 8, 8), (1, -2, 8, 8), (1, 2, -8, 8), (1, 2, 8, -8)):
        assert lib.mrcnn_mask_boundary_workspace_bytes(*bad) == 0
    assert lib.mrcnn_mask_boundary_workspace_bytes(1 << 15, 1 << 15, 1 << 10, 1 << 10) == 2 * (1 << 16) * (1 << 14) * 8       # 64-bit sizes


def test_boundary_argument_errors_are_reported_before_any_launch():
    lib = _lib()
    buf = (ctypes.c_char * 4096)()
    P = ctypes.cast(buf, ctypes.c_void_p)            # non-null stand-ins: every call below must be rejected before a launch
    N = None
    ws = lib.mrcnn_mask_boundary_workspace_bytes(3, 2, 10, 70)

    def counts(a=P, Da=3, la=N, b=P, Db=2, lb=N, H=10, W=70, d=2, w=P, wb=ws, inter=P, aa=P, ab=P, binter=P, ba=P, bb=P):
        return lib.mrcnn_mask_boundary_iou_counts_u8(a, Da, la, b, Db, lb, H, W, d, w, wb, inter, aa, ab, binter, ba, bb, N)

    wsw = lib.mrcnn_mask_boundary_workspace_bytes(3, 0, 10, 70)

    def words(m=P, D=3, H=10, W=70, d=2, w=P, wb=wsw, out=P):
        return lib.mrcnn_mask_boundary_words_u8(m, D, H, W, d, w, wb, out, N)

    for kw in (dict(Da=-1), dict(Db=-2), dict(H=-5), dict(W=-5)):
        assert counts(**kw) == -1 and b'negative' in lib.mrcnn_last_error() and b'mask_boundary_iou_counts' in lib.mrcnn_last_error()
    for kw in (dict(D=-1), dict(H=-5), dict(W=-5)):
        assert words(**kw) == -1 and b'negative' in lib.mrcnn_last_error() and b'mask_boundary_words' in lib.mrcnn_last_error()
    for f in (counts, words):
        assert f(d=0) == -1 and b'dilation' in lib.mrcnn_last_error()
        assert f(d=-3) == -1
        assert f(d=64) == -2 and b'dilation' in lib.mrcnn_last_error()
        assert f(H=50000, W=50000) == -2 and b'2^31' in lib.mrcnn_last_error()
        assert f(wb=(ws if f is counts else wsw) - 1) == -3 and b'workspace' in lib.mrcnn_last_error()
        assert f(w=N) == -3
    assert counts(la=P) == -1 and b'label' in lib.mrcnn_last_error()
    assert counts(lb=P) == -1
    for kw in (dict(a=N), dict(b=N), dict(inter=N), dict(aa=N), dict(ab=N), dict(binter=N), dict(ba=N), dict(bb=N)):
        assert counts(**kw) == -1 and b'null' in lib.mrcnn_last_error(), kw
    for kw in (dict(m=N), dict(out=N)):
        assert words(**kw) == -1 and b'null' in lib.mrcnn_last_error(), kw
    # an empty side needs neither its masks nor the intersections; the workspace check still applies to the other side
    assert counts(Db=0, b=N, inter=N, binter=N, ab=N, bb=N, wb=lib.mrcnn_mask_boundary_workspace_bytes(3, 0, 10, 70) - 8) == -3
    assert counts(Da=0, a=N, inter=N, binter=N, aa=N, ba=N, wb=0) == -3
    # nothing at all to do: returns 0 without touching a device
    assert lib.mrcnn_mask_boundary_iou_counts_u8(N, 0, N, N, 0, N, 10, 70, 2, N, 0, N, N, N, N, N, N, N) == 0
    assert lib.mrcnn_mask_boundary_words_u8(N, 0, 10, 70, 2, N, 0, N, N) == 0
    assert lib.mrcnn_mask_boundary_words_u8(N, 3, 0, 70, 2, N, 0, N, N) == 0


def test_ops_have_no_cpu_fallback():
    import torch
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    z = torch.zeros(2, 4, 4, dtype=torch.bool)
    with pytest.raises(_hip.MrcnnHipError):
        ops.mask_boundary_iou_counts(z, z, dilation=1)
    with pytest.raises(_hip.MrcnnHipError):
        ops.mask_boundary_words(z, dilation=1)
    assert ops.BOUNDARY_MAX_DILATION == 63 and ops.BOUNDARY_BAND_ROWS >= 1


# ---- the flags ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_boundary_flag():
    import evaluate
    from chainer_maskrcnn.inference_options import boundary_iou_types
    assert evaluate.build_parser().parse_args([]).boundary == 0
    assert evaluate.build_parser().parse_args(['--boundary', '1']).boundary == 1
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(['--boundary', '2'])
    assert boundary_iou_types(0) == ('segm', 'bbox') and boundary_iou_types(1) == ('segm', 'bbox', 'boundary')
    with pytest.raises(ValueError, match='--boundary must be 0 or 1'):
        boundary_iou_types(2)


def test_train_eval_boundary_flag_and_refusals():
    import train
    for kp in (False, True):
        assert train.build_parser(keypoints=kp).parse_args([]).eval_boundary == 0
    ok = train.build_parser().parse_args(['--eval-interval', '5', '--eval-metric', 'mask_coco', '--eval-boundary', '1'])
    assert ok.eval_boundary == 1
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(['--eval-boundary', '3'])
    for metric in ('mask_voc', None):                                                       # None: the default metric
        argv = ['--eval-interval', '5', '--eval-boundary', '1'] + (['--eval-metric', metric] if metric else [])
        with pytest.raises(ValueError, match='--eval-boundary 1.*--eval-metric mask_coco'):
            train.run(train.build_parser().parse_args(argv))
    with pytest.raises(ValueError, match='--eval-boundary 1.*--eval-interval'):
        train.run(train.build_parser().parse_args(['--eval-metric', 'mask_coco', '--eval-boundary', '1']))
    with pytest.raises(ValueError, match='--eval-boundary 1.*keypoint'):                    # train_keypoints.py
        train.run(train.build_parser(keypoints=True).parse_args(['--eval-interval', '5', '--eval-metric', 'keypoint_coco',
                                                                 '--eval-boundary', '1']), keypoints=True)


def test_train_keypoints_script_refuses_the_flag(monkeypatch):
    import train_keypoints
    monkeypatch.setattr(sys, 'argv', ['train_keypoints.py', '--eval-interval', '5', '--eval-metric', 'keypoint_coco', '--eval-boundary', '1'])
    with pytest.raises(ValueError, match='--eval-boundary 1'):
        train_keypoints.main()
