"""Mask-IoU counts on the device (csrc/evaluate.hip through ops.mask_iou_counts) equal NumPy's integer counts exactly, and the
streaming InstanceSegmentationVOCEvaluator equals the CPU restatement of ChainerCV (test_evaluations_cpu.py) on predict()'s outputs;
train.py --eval-interval logs validation/main/map without perturbing training."""
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
from test_evaluations_cpu import ref_eval  # noqa: E402

DEV = 'cuda:0'


def _np_counts(a, b):
    """Exact (inter, area_a, area_b) in int64: float32 products over pixel slabs of 2^18 (partial sums stay exact)."""
    hw = int(np.prod(a.shape[1:]))
    a2, b2 = a.reshape(len(a), hw) != 0, b.reshape(len(b), hw) != 0
    inter = np.zeros((len(a), len(b)), np.int64)
    for c in range(0, a2.shape[1], 1 << 18):
        inter += np.rint(a2[:, c:c + (1 << 18)].astype(np.float32) @ b2[:, c:c + (1 << 18)].astype(np.float32).T).astype(np.int64)
    return inter, a2.sum(1), b2.sum(1)


def _masks(rs, D, H, W, density):
    """Random masks: a mix of blobs (rectangles), sparse noise and all-zero / all-one rows when D allows."""
    m = rs.rand(D, H, W) < density
    for d in range(D):
        y0, x0 = rs.randint(0, H), rs.randint(0, W)
        m[d, y0:y0 + rs.randint(1, H + 1), x0:x0 + rs.randint(1, W + 1)] = True
    if D >= 3:
        m[0] = False
        m[1] = True
    return m.astype(np.uint8) * rs.randint(1, 256, size=m.shape).astype(np.uint8)        # any nonzero byte is a set pixel


def _check(a, b, la=None, lb=None, a_dev=None, b_dev=None):
    a_dev = torch.from_numpy(a).to(DEV) if a_dev is None else a_dev
    b_dev = torch.from_numpy(b).to(DEV) if b_dev is None else b_dev
    lab = lambda x: None if x is None else torch.from_numpy(x.astype(np.int32)).to(DEV)
    inter, area_a, area_b = ops.mask_iou_counts(a_dev, b_dev, lab(la), lab(lb))
    assert inter.dtype == area_a.dtype == area_b.dtype == torch.int32 and inter.shape == (len(a), len(b))
    wi, wa, wb = _np_counts(a, b)
    if la is not None:
        wi = np.where(la[:, None] == lb[None, :], wi, 0)
    np.testing.assert_array_equal(area_a.cpu().numpy(), wa)
    np.testing.assert_array_equal(area_b.cpu().numpy(), wb)
    np.testing.assert_array_equal(inter.cpu().numpy(), wi)
    return inter, area_a, area_b


@pytest.mark.parametrize('H,W,Da,Db', [(1, 1, 3, 4), (3, 5, 7, 5), (375, 500, 9, 6), (480, 640, 5, 4), (1024, 1024, 3, 2),
                                       (1, 1, 1, 1), (1024, 1024, 1, 1), (375, 500, 100, 20), (375, 500, 0, 3), (375, 500, 4, 0),
                                       (7, 9, 0, 0), (1, 63, 17, 33), (1, 1025, 5, 3)])
@pytest.mark.parametrize('labels', [False, True])
def test_counts_equal_numpy(H, W, Da, Db, labels):
    rs = np.random.RandomState(H * 7 + W + Da * 3 + Db)
    a, b = _masks(rs, Da, H, W, 0.3), _masks(rs, Db, H, W, 0.5)
    if Da and Db:
        b[-1] = a[-1]                                   # one identical pair
    if labels:
        la, lb = rs.randint(0, 4, Da), rs.randint(0, 4, Db)
        inter_l = _check(a, b, la, lb)[0].cpu().numpy()
        inter_u = _check(a, b)[0].cpu().numpy()
        same = la[:, None] == lb[None, :]
        np.testing.assert_array_equal(inter_l[same], inter_u[same])
        assert (inter_l[~same] == 0).all()
    else:
        _check(a, b)


def test_misaligned_rows_and_bool_views():
    """Rows that start at every offset mod 16 (a tensor viewed 1..15 bytes into its allocation), and torch.bool input of (D, HW)."""
    rs = np.random.RandomState(5)
    H, W = 37, 41
    a, b = _masks(rs, 6, H, W, 0.4), _masks(rs, 5, H, W, 0.4)
    for off in (1, 3, 8, 15):
        buf = torch.full((off + a.size,), 255, dtype=torch.uint8, device=DEV)          # set bytes around the view must not count
        buf2 = torch.full((off + a.size + 64,), 255, dtype=torch.uint8, device=DEV)
        av = buf[off:].view(a.shape)
        av.copy_(torch.from_numpy(a))
        bv = buf2[off:off + b.size].view(b.shape)
        bv.copy_(torch.from_numpy(b))
        _check(a, b, a_dev=av, b_dev=bv)
    _check(a, b, a_dev=torch.from_numpy(a != 0).to(DEV).reshape(6, -1), b_dev=torch.from_numpy(b != 0).to(DEV).reshape(5, -1))


def test_masks_from_mask_paste_and_repeatability():
    rs = np.random.RandomState(11)
    D, S, Cm, H, W = 40, 14, 81, 375, 500
    logits = torch.from_numpy(rs.standard_normal((D, S, S, Cm)).astype(np.float32) * 3).to(DEV)
    y0, x0 = rs.uniform(0, H - 20, D), rs.uniform(0, W - 20, D)
    bbox = np.stack([y0, x0, np.minimum(y0 + rs.uniform(5, 300, D), H), np.minimum(x0 + rs.uniform(5, 300, D), W)], 1).astype(np.float32)
    label = rs.randint(0, 80, D).astype(np.int32)
    pasted = ops.mask_paste(logits, torch.from_numpy(label).to(DEV), torch.from_numpy(bbox).to(DEV), (H, W))
    p = pasted.bool()
    gt = p[::3].clone()
    first = _check(p.cpu().numpy().astype(np.uint8), gt.cpu().numpy().astype(np.uint8), label, label[::3], a_dev=p, b_dev=gt)
    second = ops.mask_iou_counts(p, gt, torch.from_numpy(label).to(DEV), torch.from_numpy(label[::3].copy()).to(DEV))
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    assert int(first[1].sum()) > 0


# ---- the evaluator -----------------------------------------------------------------------------------------------------------------
def _reduced_model():
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=5, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.0125                         # random weights: ~uniform class probabilities (1/81 = 0.0123)
    return m


def test_streaming_evaluator_equals_the_cpu_restatement():
    from chainer_maskrcnn.evaluator import InstanceSegmentationVOCEvaluator, SyntheticEvalDataset
    m = _reduced_model()
    data = SyntheticEvalDataset(3, 120, 150, n_fg_class=80, G=6)
    names = ['c%d' % l for l in range(80)]
    for use07 in (False, True):
        got = InstanceSegmentationVOCEvaluator(data, m, label_names=names, use_07_metric=use07).evaluate()
        assert m.train is True and m.score_thresh == 0.0125 and m.nms_thresh == 0.3       # preset untouched, training state restored
        masks, labels, scores = m.predict([torch.from_numpy(data[i][0]) for i in range(len(data))])
        assert sum(int(l.shape[0]) for l in labels) > 0
        want = ref_eval([x.cpu().numpy() for x in masks], [x.cpu().numpy() for x in labels], [x.cpu().numpy() for x in scores],
                        [data[i][1].astype(bool) for i in range(len(data))], [data[i][2] for i in range(len(data))], use_07_metric=use07)
        ap = np.array([got['main/ap/%s' % n] for n in names])
        want_ap = np.full(80, np.nan)
        want_ap[:len(want['ap'])] = want['ap']
        np.testing.assert_array_equal(ap, want_ap)
        np.testing.assert_array_equal(got['main/map'], want['map'])


class _Fixed(object):
    """A 'model' whose predict() returns the given (masks, labels, scores) of each image in turn, as device tensors."""

    def __init__(self, preds):
        self.preds, self.i, self.train, self.device = preds, 0, True, torch.device(DEV)

    def predict(self, imgs):
        m, l, s = self.preds[self.i]
        self.i += 1
        return ([torch.from_numpy(m != 0).to(DEV)], [torch.from_numpy(np.asarray(l, np.int32)).to(DEV)],
                [torch.from_numpy(np.asarray(s, np.float32)).to(DEV)])


def test_ground_truth_as_predictions_gives_map_one():
    from chainer_maskrcnn.evaluator import InstanceSegmentationVOCEvaluator, SyntheticEvalDataset
    data = SyntheticEvalDataset(4, 96, 128, n_fg_class=10, G=5)
    gt = [(data[i][1], data[i][2], np.linspace(1, 0.5, len(data[i][2]))) for i in range(len(data))]
    r = InstanceSegmentationVOCEvaluator(data, _Fixed(gt), label_names=[str(l) for l in range(10)]).evaluate()
    assert r['main/map'] == 1.0
    assert all(np.isnan(v) or v == 1.0 for v in r.values())
    # an image without ground truth (G = 0): its detections, scored above all others, are false positives only
    empty = (data[0][0], np.zeros((0, 96, 128), np.uint8), np.zeros((0,), np.int32))
    extra = (data[0][1], data[0][2], np.full(len(data[0][2]), 2.0))
    fp = InstanceSegmentationVOCEvaluator([data[i] for i in range(len(data))] + [empty], _Fixed(gt + [extra])).evaluate()
    assert 0 < fp['main/map'] < 1.0


# ---- train.py --eval-interval ------------------------------------------------------------------------------------------------------
def _args(out, extra):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', '4', '--batch-size', '1', '--image-size', '256', '320',
                                            '--log-interval', '2', '--snapshot-interval', '4', '--label_file', '/nonexistent'] + extra)


def test_train_eval_interval_logs_map_and_does_not_perturb_training(tmp_path):
    import train
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    train.run(_args(a, ['--eval-interval', '2', '--eval-images', '2']))
    train.run(_args(b, []))
    la = [json.loads(l) for l in open(os.path.join(a, 'log'))]
    lb = [json.loads(l) for l in open(os.path.join(b, 'log'))]
    assert [e['iteration'] for e in la] == [2, 4] == [e['iteration'] for e in lb]
    for e in la:
        assert 'validation/main/map' in e
        v = e['validation/main/map']
        assert v is None or np.isnan(v) or 0.0 <= v <= 1.0
    assert not any(k.startswith('validation/') for e in lb for k in e)
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    for x, y in zip(la, lb):
        assert x['main/loss'] == y['main/loss']
