"""GPU tests of test-time augmentation (csrc/tta.hip, MaskRCNN.use_test_augmentation): every new kernel against the single-view kernel it
extends or a NumPy restatement, the union class NMS against oracle.predict.suppress, and the TTA path of predict / predict_keypoints end to
end on the reduced networks of test_predict_gpu.py and test_keypoint_predict_gpu.py: one unmirrored view gives predict()'s bits, hflip
equals a reference composed from the public single-view pieces, and a mirrored image gives the mirrored detections."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import predict as op
from tests import predict_judge as pj
from tests import predict_reference as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402

DEV = 'cuda:0'
F = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _eq(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(_bits(a), _bits(b))


def _np_mirror(b, W):
    b = np.asarray(b, F)
    return np.stack([b[:, 0], F(W) - b[:, 3], b[:, 2], F(W) - b[:, 1]], 1).astype(F)


# ---- kernels --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,H,W,oh,ow', [(3, 7, 9, 13, 17), (3, 50, 61, 20, 23), (3, 5, 1, 7, 1), (3, 6, 1, 3, 4), (1, 33, 45, 33, 45)])
def test_resize_mirror_equals_resize_of_the_flipped_image(C, H, W, oh, ow):
    img = _t((np.random.RandomState(H * W).rand(C, H, W) * 255).astype(F))
    _eq(ops.image_resize_mirror_f32(img, oh, ow, 0, 255.0), ops.image_resize_f32(img, oh, ow, 255.0))
    _eq(ops.image_resize_mirror_f32(img, oh, ow, 1, 255.0), ops.image_resize_f32(img.flip(-1).contiguous(), oh, ow, 255.0))


def _case(seed, R, n_class=81, ld=96, loc0=88):
    rs = np.random.RandomState(seed)
    c = rs.uniform(50, 550, (R, 2)); hw = np.exp(rs.uniform(np.log(20), np.log(300), (R, 2)))
    rois = np.concatenate([c - hw / 2, c + hw / 2], 1).astype(F)
    box = np.zeros((R, ld), F)
    box[:, :n_class] = rs.standard_normal((R, n_class)) * 3
    box[:, loc0:loc0 + 4] = rs.standard_normal((R, 4)) * 0.5
    return _t(rois), _t(box)


def test_decode_three_views():
    size, mean, std = (480, 500), (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
    views = [_case(1, 300) + (False, 1.25), _case(2, 0) + (False, 0.7), _case(3, 200) + (True, 0.8)]
    cb, pb = ops.tta_detect_decode([v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views], 81, 88,
                                   mean, std, size)
    assert cb.shape == (500, 4) and pb.shape == (500, 81)
    c0, p0 = ops.detect_decode(views[0][0], views[0][1], 81, 88, 1.25, mean, std, size)
    _eq(cb[:300], c0)
    _eq(pb[:300], p0)
    c2, p2 = ops.detect_decode(views[2][0], views[2][1], 81, 88, 0.8, mean, std, size)
    np.testing.assert_array_equal(cb[300:].cpu().numpy().view(np.int32), _np_mirror(c2.cpu().numpy(), 500).view(np.int32))
    _eq(pb[300:], p2)


def _keep_lists(keep_idx, keep_cnt, lb, le):
    cnt = keep_cnt.cpu().numpy()
    return cnt, [keep_idx[l, :cnt[l]].cpu().numpy() for l in range(lb, le)]


def test_union_nms_up_to_512_is_class_nms():
    rois, box = _case(1, 300)
    cb, pb = ops.detect_decode(rois, box, 81, 88, 1.25, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), (480, 500))
    for thresh in (0.05, 0.3):
        a = _keep_lists(*ops.class_nms(cb, pb, 1, 80, thresh, 0.3), 1, 80)
        b = _keep_lists(*ops.class_nms_ws(cb, pb, 1, 80, thresh, 0.3), 1, 80)
        np.testing.assert_array_equal(a[0], b[0])
        for x, y in zip(a[1], b[1]):
            np.testing.assert_array_equal(x, y)
        assert a[0].sum() > 0


def _union_case(seed, R, n_class, thresh):
    rs = np.random.RandomState(seed)
    c = rs.uniform(0, 400, (R, 2)); hw = np.exp(rs.uniform(np.log(4), np.log(120), (R, 2)))
    box = np.concatenate([c - hw / 2, c + hw / 2], 1).astype(F)
    dup = rs.rand(R) < 0.1                                        # duplicate boxes
    box[dup] = box[rs.randint(0, R, int(dup.sum()))]
    prob = rs.rand(R, n_class).astype(F)
    prob = (np.round(prob * 64) / 64).astype(F)                    # many duplicate scores
    at = rs.rand(R, n_class) < 0.05
    prob[at] = F(thresh)                                          # exactly at the threshold: not a candidate
    return box, prob


@pytest.mark.parametrize('R', [513, 1200, 4096])
def test_union_nms_equals_the_oracle(R):
    n_class = 6 if R == 4096 else 12
    thresh = 0.25
    box, prob = _union_case(R, R, n_class, thresh)
    for predict_mask in (True, False):
        le = n_class - 1 if predict_mask else n_class
        keep_idx, keep_cnt = ops.class_nms_ws(_t(box), _t(prob), 1, le, thresh, 0.3)
        cnt = keep_cnt.cpu().numpy()
        assert cnt[0] == 0 and (predict_mask is False or cnt[n_class - 1] == 0)
        got = np.concatenate([keep_idx[l, :cnt[l]].cpu().numpy() for l in range(1, le)])
        lab = np.concatenate([np.full(cnt[l], l - 1) for l in range(1, le)])
        want_idx, want_lab = op.suppress(box, prob, n_class, 0.3, thresh, predict_mask=predict_mask)
        np.testing.assert_array_equal(got, want_idx)
        np.testing.assert_array_equal(lab, want_lab)
        assert len(got) > 100 and (prob[:, 1:le] > thresh).sum() > 0.5 * R


def test_union_nms_refuses_more_than_4096():
    box, prob = _union_case(0, 4097, 3, 0.5)
    with pytest.raises(Exception, match='4096'):
        ops.class_nms_ws(_t(box), _t(prob), 1, 2, 0.5, 0.3)


def _mask_case(seed, D, V, S=28, Cm=96, H=97, W=131):
    rs = np.random.RandomState(seed)
    logits = [(rs.standard_normal((D, S, S, Cm)) * 2).astype(F) for _ in range(V)]
    label = rs.randint(0, 79, D).astype(np.int32)
    y0 = rs.uniform(0, H - 30, D); x0 = rs.uniform(0, W - 30, D)
    bbox = np.stack([y0, x0, np.minimum(y0 + rs.uniform(5, 80, D), H), np.minimum(x0 + rs.uniform(5, 90, D), W)], 1).astype(F)
    if D:
        bbox[0] = [3.2, 4.7, 3.9, 60.0]                             # zero-height box
    return logits, label, bbox, (H, W)


def np_mask_merge(logits, mirrors, label):
    D = len(label)
    acc = None
    for lg, mr in zip(logits, mirrors):
        z = lg[np.arange(D), :, :, label] if D else np.zeros((0,) + lg.shape[1:3], F)
        if mr:
            z = z[:, :, ::-1]
        p = (F(1) / (F(1) + np.exp(-z.astype(F)))).astype(F)
        acc = p if acc is None else (acc + p).astype(F)
    return (acc / F(len(logits))).astype(F)


def np_paste_prob(prob, bbox, size):
    """oracle.predict.paste_masks from probabilities (no sigmoid)."""
    out = np.zeros((len(bbox),) + tuple(size), bool)
    for i, b in enumerate(bbox):
        w, h = int(b[3] - b[1]), int(b[2] - b[0])
        if w <= 0 or h <= 0:
            continue
        mm = (op.cv2_resize_linear_f32(prob[i], (w, h)) * F(255)).astype(np.uint8) > 127
        s, t = int(b[0]), int(b[1])
        hh, ww = min(h, size[0] - s), min(w, size[1] - t)
        out[i, s:s + hh, t:t + ww] = mm[:hh, :ww]
    return out


def test_mask_merge_one_view_is_mask_paste():
    logits, label, bbox, size = _mask_case(2, 9, 1)
    lg, lb, bb = _t(logits[0]), _t(label), _t(bbox)
    got = ops.mask_paste_prob(ops.tta_mask_merge([lg], [False], lb), bb, size)
    _eq(got, ops.mask_paste(lg, lb, bb, size))
    assert got[1:].any() and not got[0].any()
    z = ops.tta_mask_merge([lg[:0]], [False], lb[:0])
    assert z.shape == (0, 28, 28) and ops.mask_paste_prob(z, bb[:0], size).shape == (0,) + size


@pytest.mark.parametrize('mirrors', [(False, True), (False, True, False), (True, True, False)])
def test_mask_merge_several_views_equals_numpy(mirrors):
    logits, label, bbox, size = _mask_case(len(mirrors) + 5 * mirrors[0], 11, len(mirrors))
    p = ops.tta_mask_merge([_t(l) for l in logits], list(mirrors), _t(label))
    want_p = np_mask_merge(logits, mirrors, label)
    np.testing.assert_allclose(p.cpu().numpy(), want_p, rtol=0, atol=2e-7)
    got = ops.mask_paste_prob(p, _t(bbox), size).cpu().numpy().astype(bool)
    # every pixel against float64 from the device's merged probabilities (tests/predict_judge.py); no expf: the float32 oracle's bits too
    p_dev = p.cpu().numpy()
    r64 = ref.paste(p_dev, bbox, size, False)
    band, _ = pj.paste_band(r64, ref.paste_f32(p_dev, bbox, size, False))
    n_in, n_band = pj.paste_counts(ref.paste(want_p, bbox, size, False), band)       # the condition, from the NumPy merge alone
    assert n_band <= max(1, 1e-4 * n_in) and band < 1e-3
    pj.check_paste(got, r64, band)
    np.testing.assert_array_equal(got, np_paste_prob(p_dev, bbox, size))
    assert got[1:].any() and not got[0].any()


def np_keypoint_merge(heat, mirrors, K, perm):
    acc = None
    for h, mr in zip(heat, mirrors):
        x = h
        if mr:
            x = h[:, :, ::-1, :].copy()
            x[..., :K] = x[..., np.asarray(perm)]
        acc = x.astype(F) if acc is None else (acc + x).astype(F)
    return (acc / F(len(heat))).astype(F)


@pytest.mark.parametrize('mirrors', [(False,), (False, True), (True, False, True)])
def test_keypoint_merge_equals_numpy(mirrors):
    from chainer_maskrcnn.dataset import augment
    perm = augment.flip_permutation(augment.COCO_KEYPOINT_NAMES)
    rs = np.random.RandomState(len(mirrors))
    heat = [(rs.standard_normal((5, 56, 56, 32)) * 4).astype(F) for _ in mirrors]
    got = ops.tta_keypoint_merge([_t(h) for h in heat], list(mirrors), 17, perm)
    if len(mirrors) == 1:
        np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), heat[0].view(np.int32))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), np_keypoint_merge(heat, mirrors, 17, perm).view(np.int32))
    assert ops.tta_keypoint_merge([_t(h[:0]) for h in heat], list(mirrors), 17, perm).shape == (0, 56, 56, 32)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _mask_model():
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=5, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.0125                         # random weights: ~uniform class probabilities (1/81 = 0.0123)
    return m


def _keypoint_model():
    m = MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', n_mask_convs=2, device=DEV, seed=7,
                 _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.3
    return m


def _imgs():
    rs = np.random.RandomState(0)
    return [torch.from_numpy((rs.rand(3, 120, 150) * 255).astype(F)), torch.from_numpy((rs.rand(3, 100, 100) * 255).astype(F))]


def test_one_view_is_predict():
    m = _mask_model()
    imgs = _imgs()
    masks, labels, scores = m.predict(imgs)
    bboxes = m.last_bboxes
    m.use_test_augmentation([m.min_size])
    masks2, labels2, scores2 = m.predict(imgs)
    assert isinstance(m.last_rois, list) and m.train is True          # the TTA path ran
    for i in range(2):
        _eq(masks2[i], masks[i])
        _eq(labels2[i], labels[i])
        _eq(scores2[i], scores[i])
        _eq(m.last_bboxes[i], bboxes[i])
    assert sum(int(l.shape[0]) for l in labels) > 0 and any(bool(mk.any()) for mk in masks)


def test_one_view_is_predict_keypoints():
    from chainer_maskrcnn.evaluator import SyntheticKeypointEvalDataset
    m = _keypoint_model()
    data = SyntheticKeypointEvalDataset(2, 120, 150)
    imgs = [torch.from_numpy(data[i][0]) for i in range(2)]
    out = m.predict_keypoints(imgs, return_heatmaps=True)
    bboxes = m.last_bboxes
    m.use_test_augmentation([m.min_size])
    out2 = m.predict_keypoints(imgs, return_heatmaps=True)
    assert isinstance(m.last_rois, list)
    for a, b in zip(out, out2):
        for i in range(2):
            _eq(b[i], a[i])
    for i in range(2):
        _eq(m.last_bboxes[i], bboxes[i])
    assert sum(int(l.shape[0]) for l in out[1]) > 0


def _reference_views(m, img, views):
    """The public single-view pieces per view: prepare (of the mirrored image), forward, detect_decode, NumPy mirror.  Returns the union
    (boxes, probs, levels, view ids) on the host and per view (features, scale, mirror)."""
    from chainer_maskrcnn.nn import core
    H, W = img.shape[1:]
    keep = m.train, core.TRAIN, m.min_size, m.max_size
    m.train, core.TRAIN = False, False
    out, per = [], []
    try:
        for v, (s, mirror) in enumerate(views):
            m.min_size = s
            x = m.prepare((img.flip(-1) if mirror else img).to(DEV).contiguous())
            scale = x.shape[2] / W
            _, _, rois, _, levels = m(x[None].contiguous(), scale=scale)
            cb, pb = ops.detect_decode(rois.contiguous(), m.head.last_box_out, m.n_class, m.head.LOC0, scale, m.loc_normalize_mean,
                                       m.loc_normalize_std, (H, W))
            cb = cb.cpu().numpy()
            out.append((_np_mirror(cb, W) if mirror else cb, pb.cpu().numpy(), levels.cpu().numpy(), np.full(len(cb), v)))
            per.append((m.head.x, scale, mirror))
    finally:
        m.train, core.TRAIN, m.min_size, m.max_size = keep
    return [np.concatenate([o[j] for o in out]) for j in range(4)], per


def _reference_branch(m, bbox, level, view, per, W):
    from chainer_maskrcnn.nn import core
    keep = m.train, core.TRAIN
    m.train, core.TRAIN = False, False
    res = []
    try:
        for u, (feats, scale, mirror) in enumerate(per):
            b = (_np_mirror(bbox, W) if mirror else bbox) * F(scale)
            lv = ops.map_rois_to_fpn_levels(_t(b.astype(F))).clamp(0, len(feats) - 1).cpu().numpy()
            lv = np.where(view == u, level, lv)
            xy5 = np.concatenate([np.zeros((len(b), 1), F), b[:, [1, 0, 3, 2]]], 1).astype(F)
            res.append(m.head.mask_branch(feats, _t(xy5), _t(lv.astype(np.int32)), m.extractor.spatial_scales).cpu().numpy())
    finally:
        m.train, core.TRAIN = keep
    return res


@pytest.mark.parametrize('sizes', [[160], [160, 224]])
def test_hflip_equals_the_composed_reference(sizes):
    m = _mask_model()
    img = _imgs()[0]
    H, W = img.shape[1:]
    m.use_test_augmentation(sizes, hflip=True)
    masks, labels, scores = m.predict([img])
    (cls, prob, lev, view), per = _reference_views(m, img, [(s, mr) for s in sizes for mr in (False, True)])
    R = len(cls)
    assert m.last_decoded[0].shape[0] == R
    np.testing.assert_array_equal(m.last_decoded[0].cpu().numpy().view(np.int32), cls.view(np.int32))
    np.testing.assert_array_equal(m.last_decoded[1].cpu().numpy().view(np.int32), prob.view(np.int32))
    if len(sizes) > 1:
        assert R > 512                                                  # the union path of class_nms_ws
    idx, lab = op.suppress(cls, prob, m.n_class, m.nms_thresh, m.score_thresh, predict_mask=True)
    assert len(idx) > 0
    np.testing.assert_array_equal(m.last_bboxes[0].cpu().numpy().view(np.int32), cls[idx].view(np.int32))
    np.testing.assert_array_equal(labels[0].cpu().numpy(), lab)
    np.testing.assert_array_equal(scores[0].cpu().numpy().view(np.int32), prob[idx, lab + 1].view(np.int32))
    logits = _reference_branch(m, cls[idx], lev[idx], view[idx], per, W)
    p = np_mask_merge(logits, [mr for _, _, mr in per], lab)
    want = np_paste_prob(p, cls[idx], (H, W))
    got = masks[0].cpu().numpy()
    assert (got != want).mean() < 1e-4 and got.any()


def test_keypoint_hflip_equals_the_numpy_merge():
    from chainer_maskrcnn.dataset import augment
    from chainer_maskrcnn.evaluator import SyntheticKeypointEvalDataset
    perm = augment.flip_permutation(augment.COCO_KEYPOINT_NAMES)
    m = _keypoint_model()
    img = torch.from_numpy(SyntheticKeypointEvalDataset(1, 120, 150)[0][0])
    W = img.shape[2]
    m.use_test_augmentation([160], hflip=True, keypoint_flip_perm=perm)
    kps, labels, scores, heat = m.predict_keypoints([img], return_heatmaps=True)
    (cls, prob, lev, view), per = _reference_views(m, img, [(160, False), (160, True)])
    idx, lab = op.suppress(cls, prob, m.n_class, m.nms_thresh, m.score_thresh, predict_mask=False)
    D = len(idx)
    assert D > 0
    np.testing.assert_array_equal(m.last_bboxes[0].cpu().numpy().view(np.int32), cls[idx].view(np.int32))
    np.testing.assert_array_equal(labels[0].cpu().numpy(), lab)
    hv = _reference_branch(m, cls[idx], lev[idx], view[idx], per, W)
    merged = np_keypoint_merge(hv, [False, True], 17, perm)
    np.testing.assert_array_equal(heat[0].cpu().numpy().view(np.int32),
                                  np.ascontiguousarray(merged[..., :17].transpose(0, 3, 1, 2)).reshape(D, 17, -1).view(np.int32))
    want = ops.keypoint_decode(_t(merged), _t(cls[idx]), 17)
    _eq(kps[0], want)


def test_mirror_symmetry():
    m = _mask_model()
    img = _imgs()[0]
    W = img.shape[2]
    m.use_test_augmentation([160, 200], hflip=True)
    _, la, sa = m.predict([img])
    ba = m.last_bboxes[0].cpu().numpy()
    _, lb, sb = m.predict([img.flip(-1).contiguous()])
    bb = _np_mirror(m.last_bboxes[0].cpu().numpy(), W)
    la, sa, lb, sb = (t.cpu().numpy() for t in (la[0], sa[0], lb[0], sb[0]))
    assert len(la) > 0 and len(la) == len(lb)
    oa, ob = np.lexsort((ba[:, 0], sa, la)), np.lexsort((bb[:, 0], sb, lb))
    np.testing.assert_array_equal(la[oa], lb[ob])
    np.testing.assert_array_equal(sa[oa], sb[ob])
    assert np.abs(ba[oa] - bb[ob]).max() <= 1e-3 * W


def test_evaluator_with_one_view_is_unchanged():
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, SyntheticCOCOEvalDataset
    m = _mask_model()
    data = SyntheticCOCOEvalDataset(2, 120, 150, n_fg_class=80)
    a = InstanceSegmentationCOCOEvaluator(data, m)
    ra = a.evaluate()
    m.use_test_augmentation([m.min_size])
    b = InstanceSegmentationCOCOEvaluator(data, m)
    rb = b.evaluate()
    assert ra == rb and a.stats == b.stats


def test_evaluate_cli_writes_the_tta_key(tmp_path):
    import evaluate
    out = str(tmp_path / 'ev')
    args = evaluate.build_parser().parse_args(['--synthetic', '1', '--eval-images', '1', '--image-size', '96', '128', '--tta-hflip', '1',
                                               '--tta-sizes', '96', '128', '--tta-max-size', '200', '--no-results', '--out', out])
    stats = evaluate.run(args)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert got['tta'] == {'sizes': [96, 128], 'hflip': True, 'max_size': 200}
    assert set(stats) == {'segm', 'bbox'} and got['segm'] == stats['segm']
