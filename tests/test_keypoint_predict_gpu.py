"""Keypoint inference on the device: the heat-map decode (csrc/keypoints.hip through ops.keypoint_decode) equals a NumPy restatement,
MaskRCNN.predict_keypoints agrees with predict and with that restatement on the head's own heat maps, KeypointCOCOEvaluator equals the
CPU restatement of COCOeval (test_keypoint_eval_cpu.py), and train_keypoints.py --eval-metric keypoint_coco logs its keys without
perturbing training."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from chainer_maskrcnn._hip import ops  # noqa: E402
from test_keypoint_eval_cpu import ref_coco_keypoint_eval  # noqa: E402
from tests import predict_cases as pc  # noqa: E402

DEV = 'cuda:0'


def np_decode(heat, bbox, K):
    """NumPy restatement of mrcnn_keypoint_decode_f32: heat (D,S,S,Cp), bbox (D,4) float32 -> idx (D,K) int, y, x, logit (D,K)
    float32, prob (D,K) float64."""
    D, S = heat.shape[0], heat.shape[1]
    h = heat[..., :K].transpose(0, 3, 1, 2).reshape(D, K, S * S)           # the reference's (D, K, S*S) heat maps
    idx = h.argmax(-1)
    logit = h.max(-1)
    y1, x1, y2, x2 = (bbox[:, j:j + 1] for j in range(4))
    y = (idx // S).astype(np.float32) * ((y2 - y1) / np.float32(S)) + y1
    x = (idx % S).astype(np.float32) * ((x2 - x1) / np.float32(S)) + x1
    prob = 1.0 / np.exp(h.astype(np.float64) - logit[..., None].astype(np.float64)).sum(-1)
    return idx, y, x, logit, prob


def _boxes(rs, D, H=480, W=640):
    y0, x0 = rs.uniform(0, H - 40, D), rs.uniform(0, W - 40, D)
    return np.stack([y0, x0, np.minimum(y0 + rs.uniform(3, 400, D), H), np.minimum(x0 + rs.uniform(3, 400, D), W)], 1).astype(np.float32)


@pytest.mark.parametrize('D,K', [(0, 17), (1, 17), (7, 17), (300, 17), (5, 20), (3, 1)])
def test_decode_equals_numpy(D, K):
    rs = np.random.RandomState(D * 31 + K)
    S, Cp = 56, 32
    heat = (rs.standard_normal((D, S, S, Cp)) * 4).astype(np.float32)
    heat[..., K:] = 1e4                                              # padding channels must not be read into the result
    for d in range(D):                                               # planted ties: the maximum again at later cells
        for k in range(K):
            c = rs.randint(0, S * S - 1, 3)
            v = np.float32(20 + rs.randint(0, 3))
            for ci in sorted(c):
                heat[d, ci // S, ci % S, k] = v
    if D:
        heat[0, :, :, 0] = 1.5                                       # all cells equal: index 0, prob 1 / S^2
    bbox = _boxes(rs, D)
    h_dev, b_dev = torch.from_numpy(heat).to(DEV), torch.from_numpy(bbox).to(DEV)
    out, idx = ops.keypoint_decode(h_dev, b_dev, K, return_index=True)
    assert out.shape == (D, K, 4) and out.dtype == torch.float32 and idx.shape == (D, K) and idx.dtype == torch.int32
    widx, wy, wx, wl, wp = np_decode(heat, bbox, K)
    o, i = out.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_array_equal(i, widx)
    np.testing.assert_array_equal(o[..., 0], wy)
    np.testing.assert_array_equal(o[..., 1], wx)
    np.testing.assert_array_equal(o[..., 2], wl)
    np.testing.assert_allclose(o[..., 3], wp, rtol=1e-6, atol=0)
    if D:
        assert i[0, 0] == 0 and abs(o[0, 0, 3] * S * S - 1) < 1e-6
    out2, idx2 = ops.keypoint_decode(h_dev, b_dev, K, return_index=True)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(idx2, idx)     # bit-identical repeat
    assert torch.equal(ops.keypoint_decode(h_dev, b_dev, K).view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize('S,K,Cp,D', pc.KEYPOINT_SHAPES)
def test_decode_case(S, K, Cp, D):
    """tests/predict_cases.py: every lanes-per-cell value P in {1, 2, 8, 16, 64} at every S in {7, 14, 28, 56}, the split counts 1 .. 392
    (asserted in tests/test_predict_cases_cpu.py).  Index, y, x and logit bit for bit, the probability against the float64 sum."""
    c = pc.keypoint_case(S, K, Cp, D)
    h_dev, b_dev = torch.from_numpy(c['heat']).to(DEV), torch.from_numpy(c['bbox']).to(DEV)
    out, idx = ops.keypoint_decode(h_dev, b_dev, K, return_index=True)
    assert out.shape == (D, K, 4) and out.dtype == torch.float32 and idx.shape == (D, K) and idx.dtype == torch.int32
    widx, wy, wx, wl, wp = c['want']
    o, i = out.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_array_equal(i, widx)
    np.testing.assert_array_equal(o[..., 0], wy)
    np.testing.assert_array_equal(o[..., 1], wx)
    np.testing.assert_array_equal(o[..., 2], wl)
    np.testing.assert_allclose(o[..., 3], wp, rtol=1e-6, atol=0)
    assert i[0, 0] == 0 and abs(o[0, 0, 3] * S * S - 1) < 1e-6


def test_decode_rejects_bad_arguments():
    h = torch.zeros((2, 56, 56, 32), device=DEV)
    b = torch.zeros((2, 4), device=DEV)
    with pytest.raises(ValueError):
        ops.keypoint_decode(h, b, 33)
    with pytest.raises(ValueError):
        ops.keypoint_decode(h, b[:1], 17)
    with pytest.raises(ValueError):
        ops.keypoint_decode(torch.zeros((2, 56, 56, 18), device=DEV), b, 17)
    with pytest.raises(TypeError):
        ops.keypoint_decode(h.double(), b, 17)
    # a contiguous view 4 bytes into its storage is realigned, not rejected
    flat = torch.zeros((1 + 56 * 56 * 32,), device=DEV)
    flat[1:].copy_(torch.arange(56 * 56 * 32, dtype=torch.float32, device=DEV))
    kp = ops.keypoint_decode(flat[1:].view(1, 56, 56, 32), b[:1], 17)
    assert kp[0, :, 2].tolist() == [float(56 * 56 * 32 - 32 + k) for k in range(17)]


# ---- predict_keypoints ---------------------------------------------------------------------------------------------------------------
def _keypoint_model():
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    m = MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', n_mask_convs=2, device=DEV, seed=7,
                 _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.3                             # random weights: two classes, foreground probability around 0.5
    return m


def test_predict_keypoints_matches_predict_and_the_numpy_decode():
    from chainer_maskrcnn.evaluator import SyntheticKeypointEvalDataset
    m = _keypoint_model()
    data = SyntheticKeypointEvalDataset(2, 120, 150)
    imgs = [torch.from_numpy(data[i][0]) for i in range(2)]
    _, labels, scores = m.predict(imgs)
    bboxes = [b.cpu().numpy() for b in m.last_bboxes]
    kps, labels2, scores2, heat = m.predict_keypoints(imgs, return_heatmaps=True)
    assert m.train is True
    assert sum(int(l.shape[0]) for l in labels) > 0
    for i in range(2):
        np.testing.assert_array_equal(labels2[i].cpu().numpy(), labels[i].cpu().numpy())
        np.testing.assert_array_equal(scores2[i].cpu().numpy(), scores[i].cpu().numpy())
        np.testing.assert_array_equal(m.last_bboxes[i].cpu().numpy(), bboxes[i])
        D = int(labels[i].shape[0])
        assert kps[i].shape == (D, 17, 4) and heat[i].shape == (D, 17, 56 * 56)
        h = heat[i].cpu().numpy().reshape(D, 17, 56, 56).transpose(0, 2, 3, 1)
        widx, wy, wx, wl, wp = np_decode(np.ascontiguousarray(h), bboxes[i], 17)
        o = kps[i].cpu().numpy()
        np.testing.assert_array_equal(o[..., 0], wy)
        np.testing.assert_array_equal(o[..., 1], wx)
        np.testing.assert_array_equal(o[..., 2], wl)
        np.testing.assert_allclose(o[..., 3], wp, rtol=1e-6, atol=0)
    assert list(m.predict_keypoints(imgs[:1])[0][0].shape) == [int(labels[0].shape[0]), 17, 4]


def test_predict_keypoints_refuses_a_mask_model():
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    m = MaskRCNN(n_fg_class=3, device=DEV, seed=1, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=96, max_size=128)
    with pytest.raises(ValueError, match='fpn_keypoint'):
        m.predict_keypoints([torch.zeros((3, 96, 128))])


# ---- the evaluator -------------------------------------------------------------------------------------------------------------------
class _Fixed(object):
    """A keypoint 'model' whose predict_keypoints returns the given ((D,K,2) (y, x), scores) of each image in turn, on the device."""

    def __init__(self, preds):
        self.preds, self.i, self.train, self.device = preds, 0, True, torch.device(DEV)

    def predict_keypoints(self, imgs):
        yx, s = self.preds[self.i]
        self.i += 1
        kp = np.zeros(yx.shape[:2] + (4,), np.float32)
        kp[..., :2] = yx
        return ([torch.from_numpy(kp).to(DEV)], [torch.zeros((len(s),), dtype=torch.int32, device=DEV)],
                [torch.from_numpy(np.asarray(s, np.float32)).to(DEV)])


def test_ground_truth_as_keypoints_gives_ap_one_and_displaced_ones_the_restatement():
    from chainer_maskrcnn.evaluator import KeypointCOCOEvaluator, SyntheticKeypointEvalDataset
    data = SyntheticKeypointEvalDataset(4, 160, 200, G=5)
    ex = [data[i] for i in range(len(data))]
    gt = [(e[1][:, :, :2].astype(np.float32), np.linspace(1, 0.5, len(e[1]))) for e in ex]
    r = KeypointCOCOEvaluator(ex, _Fixed(gt)).evaluate()
    assert sorted(r) == ['main/ap50', 'main/ap75', 'main/ap_large', 'main/ap_medium', 'main/ar', 'main/map']
    one = pytest.approx(1.0, abs=1e-12)                             # precision tp / (fp + tp + eps), as in COCOeval
    assert r['main/map'] == one and r['main/ap50'] == one and r['main/ar'] == 1.0
    rs = np.random.RandomState(3)
    moved = []
    for yx, s in gt:
        yx = yx.copy()
        half = rs.rand(*yx.shape[:2]) < 0.5
        yx[half] += rs.uniform(-12, 12, (int(half.sum()), 2)).astype(np.float32)
        moved.append((yx, s))
    got = KeypointCOCOEvaluator(ex, _Fixed(moved)).evaluate()
    want = ref_coco_keypoint_eval([p[0] for p in moved], [p[1] for p in moved], [e[1] for e in ex], [e[2] for e in ex],
                                  [e[3] for e in ex], [e[4] for e in ex])
    assert got['main/map'] == want['AP'] and got['main/ap50'] == want['AP50'] and got['main/ap75'] == want['AP75']
    assert got['main/ap_medium'] == want['APm'] and got['main/ap_large'] == want['APl'] and got['main/ar'] == want['AR']
    assert 0 < got['main/map'] < 1


def test_evaluator_on_the_keypoint_network():
    from chainer_maskrcnn.evaluator import KeypointCOCOEvaluator, SyntheticKeypointEvalDataset
    m = _keypoint_model()
    r = KeypointCOCOEvaluator(SyntheticKeypointEvalDataset(2, 120, 150), m).evaluate()
    assert m.train is True and m.score_thresh == 0.3
    assert all(v == -1.0 or 0.0 <= v <= 1.0 for v in r.values())


# ---- train_keypoints.py --eval-metric keypoint_coco ----------------------------------------------------------------------------------
def _args(out, extra):
    import train
    return train.build_parser(keypoints=True).parse_args(['--out', out, '--iteration', '4', '--batch_size', '1', '--image-size', '256', '320',
                                                          '--log-interval', '2', '--snapshot-interval', '4', '--min_size', '256',
                                                          '--max_size', '320'] + extra)


def test_train_keypoints_eval_logs_keypoint_ap_and_does_not_perturb_training(tmp_path):
    import train
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    train.run(_args(a, ['--eval-interval', '2', '--eval-images', '2', '--eval-metric', 'keypoint_coco']), keypoints=True)
    train.run(_args(b, []), keypoints=True)
    la = [json.loads(l) for l in open(os.path.join(a, 'log'))]
    lb = [json.loads(l) for l in open(os.path.join(b, 'log'))]
    assert [e['iteration'] for e in la] == [2, 4] == [e['iteration'] for e in lb]
    keys = ['validation/main/' + k for k in ('map', 'ap50', 'ap75', 'ap_medium', 'ap_large', 'ar')]
    for e in la:
        for k in keys:
            assert k in e and (e[k] == -1.0 or 0.0 <= e[k] <= 1.0), (k, e.get(k))
    assert not any(k.startswith('validation/') for e in lb for k in e)
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    for x, y in zip(la, lb):
        assert x['main/loss'] == y['main/loss']
