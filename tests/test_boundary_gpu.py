"""Boundary AP on the device: the boundary-band kernel (csrc/evaluate.hip through ops.mask_boundary_words) and the counts of
ops.mask_boundary_iou_counts equal the literal restatement (boundary_reference.py) bit for bit at the tile, word and band edges; the COCO
evaluator with 'boundary' leaves 'segm' / 'bbox' as they are and equals the restated COCOeval fed Boundary IoUs; evaluate.py --boundary
and train.py --eval-boundary write their keys without touching anything else."""
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

import boundary_reference as bref  # noqa: E402
import test_coco_eval_cpu as tcc  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402

DEV = 'cuda:0'
BAND = ops.BOUNDARY_BAND_ROWS
TALL = 3 * BAND + 5                             # three row bands and a remainder


def _families(H, W, d, rs):
    """The mask families of one image size as a (D, H, W) uint8 stack (set pixels carry 1 unless said otherwise)."""
    out = []

    def new():
        out.append(np.zeros((H, W), np.uint8))
        return out[-1]
    new()[:] = 1                                                   # all ones: a frame of width d
    new()                                                          # all zeros
    new()[H // 2, W // 2] = 1                                      # one pixel
    new()[0, 0] = 1
    new()[H - 1, W - 1] = 1
    hh, hw = max(H // 2, 1), max(W // 2, 1)
    new()[:hh, W // 4:W // 4 + hw] = 1                             # rectangles touching the top, bottom, left, right edge
    new()[H - hh:, W // 4:W // 4 + hw] = 1
    new()[H // 4:H // 4 + hh, :hw] = 1
    new()[H // 4:H // 4 + hh, W - hw:] = 1
    for x in (63, 64, 65):                                         # sides on a word seam and on a band seam
        for y in (BAND - 1, BAND, BAND + 1):
            new()[max(y - 40, 0):y, max(x - 50, 0):x] = 1
            new()[y:y + 70, x:x + 90] = 1
    m = new()                                                      # a blob with a one-pixel hole deeper than d from its rim
    m[1:H - 1, 1:W - 1] = 1
    m[H // 2, W // 2] = 0
    m = new()
    m[:] = 1
    m[min(d + 2, H - 1), min(d + 2, W - 1)] = 0
    new()[:] = rs.rand(H, W) < 0.9                                 # noise
    new()[:] = rs.rand(H, W) < 0.5
    new()[:] = (rs.rand(H, W) < 0.9) * 2                           # bytes 2 and 255 count as set
    new()[:] = (rs.rand(H, W) < 0.97) * np.where(rs.rand(H, W) < 0.5, 255, 2)
    return np.stack(out)


def _check_words(m_host, m_dev, d):
    words = ops.mask_boundary_words(m_dev, dilation=d)
    D, H, W = m_host.shape
    assert words.dtype == torch.int64 and words.is_cuda and tuple(words.shape) == (D, H, (W + 63) // 64)
    got, tail = bref.unpack_words(words.cpu().numpy(), W)
    assert not tail.any()
    want = bref.ref_boundaries(m_host, d)
    bad = np.argwhere(got != want)
    assert bad.size == 0, 'first wrong band pixels (mask, y, x): %s' % bad[:5].tolist()
    return got


# (H, W, d): every W of {1, 63, 64, 65, 127, 129, 200}, H of {1, 2, d, 2 d + 1, three bands and a remainder}, every d of
# {1, 2, 3, 16, 31, 32, 33, 63}, d > W and d > H; W = 600 / 1100 reach a second column group of the band kernel and a second window of a row
ROW_CASES = [(TALL, 200, 16), (TALL, 65, 3), (TALL, 129, 31), (TALL, 64, 32), (TALL, 127, 33), (TALL, 200, 63), (TALL, 63, 1), (TALL, 1, 2),
             (1, 1, 1), (1, 200, 1), (2, 63, 2), (2, 1, 3), (16, 64, 16), (33, 65, 16), (63, 127, 31), (127, 129, 63), (3, 200, 1),
             (5, 63, 2), (40, 30, 33), (32, 200, 32), (70, 600, 2), (66, 1100, 12), (2 * BAND, 128, 3)]


@pytest.mark.parametrize('H,W,d', ROW_CASES)
def test_boundary_rows_equal_the_restatement(H, W, d):
    rs = np.random.RandomState(H * 7 + W * 3 + d)
    m = _families(H, W, d, rs)
    got = _check_words(m, torch.from_numpy(m).to(DEV), d)
    if d > H or d > W:
        np.testing.assert_array_equal(got, m != 0)                # no pixel has its whole square inside the image: all set is boundary
    np.testing.assert_array_equal(got[1], False)
    if H > 2 * d and W > 2 * d:                                   # all ones: exactly the frame of width d
        frame = np.ones((H, W), bool)
        frame[d:H - d, d:W - d] = False
        np.testing.assert_array_equal(got[0], frame)


def test_boundary_rows_bool_input_and_view_at_an_odd_byte_offset():
    rs = np.random.RandomState(5)
    H, W, d = 70, 129, 3                                          # odd W: the rows start at every alignment
    m = _families(H, W, d, rs)
    _check_words(m, torch.from_numpy(m != 0).to(DEV), d)
    for off in (1, 7):
        buf = torch.full((off + m.size + 32,), 255, dtype=torch.uint8, device=DEV)      # set bytes around the view must not count
        v = buf[off:off + m.size].view(m.shape)
        v.copy_(torch.from_numpy(m))
        assert v.data_ptr() % 2 == 1
        _check_words(m, v, d)


def test_default_dilation_is_the_rule():
    m = np.zeros((2, 75, 100), np.uint8)
    m[0, 10:60, 20:90] = 1
    m[1] = 1
    got, _ = bref.unpack_words(ops.mask_boundary_words(torch.from_numpy(m).to(DEV)).cpu().numpy(), 100)
    np.testing.assert_array_equal(got, bref.ref_boundaries(m, 2))           # 0.02 * 125 = 2.5 rounds to 2


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
def _blobs(rs, D, H, W):
    m = np.zeros((D, H, W), np.uint8)
    for k in range(D):
        if k % 5 == 4:
            m[k] = rs.rand(H, W) < 0.8
            continue
        for _ in range(rs.randint(1, 3)):
            y0, x0 = rs.randint(0, H), rs.randint(0, W)
            m[k, y0:y0 + rs.randint(1, H + 1), x0:x0 + rs.randint(1, W + 1)] = rs.randint(1, 256)
    return m


def _check_counts(a, b, d, dilation):
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = ops.mask_boundary_iou_counts(ta, tb, dilation=dilation)
    Da, Db = len(a), len(b)
    assert [tuple(g.shape) for g in got] == [(Da, Db), (Da,), (Db,)] * 2 and all(g.dtype == torch.int32 and g.is_cuda for g in got)
    for g, w in zip(got, bref.ref_counts(a, b, d)):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    for g, p in zip(got[:3], ops.mask_iou_counts(ta, tb)):          # the mask counts are the plain call's
        assert torch.equal(g, p)
    for g, h in zip(got, ops.mask_boundary_iou_counts(ta, tb, dilation=dilation)):
        assert torch.equal(g, h)
    return ta, tb, got


@pytest.mark.parametrize('H,W', [(37, 70), (64, 200)])
@pytest.mark.parametrize('Da,Db', [(0, 3), (3, 0), (1, 1), (17, 5), (33, 18)])
def test_counts_equal_the_restatement(Da, Db, H, W):
    rs = np.random.RandomState(Da * 31 + Db * 7 + H)
    a, b = _blobs(rs, Da, H, W), _blobs(rs, Db, H, W)
    if Da and Db:
        b[0] = a[Da - 1]
    ta, tb, got = _check_counts(a, b, 3, 3)
    if Da > 16 and Db > 1:                                            # labels: cross-label pairs are 0 and same-label pairs unchanged
        la, lb = rs.randint(0, 3, Da).astype(np.int32), rs.randint(0, 3, Db).astype(np.int32)
        lab = ops.mask_boundary_iou_counts(ta, tb, torch.from_numpy(la).to(DEV), torch.from_numpy(lb).to(DEV), dilation=3)
        same = torch.from_numpy(la[:, None] == lb[None, :]).to(DEV)
        for k in (0, 3):
            assert torch.equal(lab[k], torch.where(same, got[k], torch.zeros_like(got[k])))
            assert int(lab[k][~same].abs().sum()) == 0 and int(got[k][~same].sum()) > 0
        for k in (1, 2, 4, 5):
            assert torch.equal(lab[k], got[k])


def test_counts_at_a_real_image_size_with_the_default_dilation():
    rs = np.random.RandomState(12)
    assert bref.ref_dilation(375, 500) == 12
    _check_counts(_blobs(rs, 20, 375, 500), _blobs(rs, 6, 375, 500), 12, None)


def test_argument_checks_of_the_ops():
    z = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    for bad in (0, 64, -1, 1.5, True):
        with pytest.raises(ValueError, match='dilation'):
            ops.mask_boundary_iou_counts(z, z, dilation=bad)
        with pytest.raises(ValueError, match='dilation'):
            ops.mask_boundary_words(z, dilation=bad)
    with pytest.raises(ValueError, match=r'\(D,H,W\)'):
        ops.mask_boundary_iou_counts(z.reshape(2, 64), z.reshape(2, 64), dilation=1)
    with pytest.raises(ValueError, match=r'\(D,H,W\)'):
        ops.mask_boundary_words(z.reshape(2, 64), dilation=1)
    with pytest.raises(ValueError):
        ops.mask_boundary_iou_counts(z, z[:, :4], dilation=1)
    with pytest.raises(ValueError, match='both label arrays'):
        ops.mask_boundary_iou_counts(z, z, a_label=torch.zeros(2, device=DEV), dilation=1)
    with pytest.raises(TypeError):
        ops.mask_boundary_words(z.float(), dilation=1)
    assert tuple(ops.mask_boundary_words(z[:0], dilation=1).shape) == (0, 8, 1)


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------
class _Shifted(object):
    """A stand-in for the model: predict() returns the given (masks, labels, scores, boxes (y1,x1,y2,x2)) of each image in turn."""

    def __init__(self, preds):
        self.preds, self.i, self.train, self.device = preds, 0, True, torch.device(DEV)

    def predict(self, imgs):
        m, l, s, b = self.preds[self.i % len(self.preds)]
        self.i += 1
        self.last_bboxes = [torch.from_numpy(np.asarray(b, np.float32)).to(DEV)]
        return ([torch.from_numpy(m != 0).to(DEV)], [torch.from_numpy(np.asarray(l, np.int32)).to(DEV)],
                [torch.from_numpy(np.asarray(s, np.float32)).to(DEV)])


def test_evaluator_with_boundary_keeps_segm_and_bbox_and_equals_the_restatement(monkeypatch):
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, SyntheticCOCOEvalDataset
    from chainer_maskrcnn.utils.synthetic import make_batch
    H, W, G = 96, 128, 5
    data = SyntheticCOCOEvalDataset(3, H, W, n_fg_class=10, G=G)
    preds, images = [], []
    for i in range(len(data)):
        _, gm, gl, ga, gc, gb, _ = data[i]
        box = make_batch(data.first_seed + i, 1, H, W, G=G, n_fg_class=10)['bboxes'][0]
        pm = np.stack([np.roll(np.asarray(gm[g]), (g % 3, 2 * (g % 2) + i), axis=(0, 1)) for g in range(G)] + [np.asarray(gm[0])])
        pl = np.concatenate([np.asarray(gl), [(int(gl[0]) + 1) % 10]]).astype(np.int32)           # the last one: a wrong label
        ps = np.linspace(0.9, 0.3, G + 1)
        preds.append((pm, pl, ps, np.concatenate([box, box[:1]])))
        gts = [{'category_id': int(gl[g]), 'area': float(ga[g]), 'iscrowd': int(gc[g]), 'mask': np.asarray(gm[g])} for g in range(G)]
        dts = [{'category_id': int(pl[k]), 'score': float(np.float32(ps[k])), 'mask': pm[k], 'area': float(np.count_nonzero(pm[k]))}
               for k in range(G + 1)]
        images.append((gts, dts))
    plain = InstanceSegmentationCOCOEvaluator(data, _Shifted(preds))
    rep0 = plain.evaluate()
    ev = InstanceSegmentationCOCOEvaluator(data, _Shifted(preds), iou_types=('segm', 'bbox', 'boundary'))
    rep = ev.evaluate()
    assert set(plain.stats) == {'segm', 'bbox'} and set(ev.stats) == {'segm', 'bbox', 'boundary'}
    assert ev.stats['segm'] == plain.stats['segm'] and ev.stats['bbox'] == plain.stats['bbox']
    assert {k: v for k, v in rep.items() if '/boundary/' not in k} == rep0
    monkeypatch.setattr(tcc, '_ref_iou', bref.ref_cocoeval_boundary_iou)
    want = tcc.ref_cocoeval(images, 'segm')
    assert ev.stats['boundary'] == want, (ev.stats['boundary'], want)
    assert 0 < want['AP'] < plain.stats['segm']['AP']              # the shifts cost the bands more than the masks
    keys = ('map', 'ap50', 'ap75', 'ap_small', 'ap_medium', 'ap_large', 'ar')
    assert {k for k in rep if '/boundary/' in k} == {'main/boundary/%s' % k for k in keys}
    assert rep['main/boundary/map'] == want['AP'] and rep['main/boundary/ar'] == want['AR100']


# ---- evaluate.py --boundary and train.py --eval-boundary --------------------------------------------------------------------------------------
def _evaluate(tmp_path, name, extra):
    import evaluate
    out = tmp_path / name
    argv = ['--synthetic', '1', '--eval-images', '2', '--image-size', '128', '160', '--score-thresh', '0.0125', '--label_file', '/nonexistent',
            '--out', str(out)] + extra
    stats = evaluate.run(evaluate.build_parser().parse_args(argv))
    return out, stats


def test_evaluate_script_boundary_flag(tmp_path, capsys):
    files = ('segm_results.json', 'bbox_results.json', 'metrics.json')
    out0, stats0 = _evaluate(tmp_path, 'default', [])
    printed0 = capsys.readouterr().out
    out1, stats1 = _evaluate(tmp_path, 'off', ['--boundary', '0'])
    printed1 = capsys.readouterr().out
    for f in files:
        assert open(out0 / f, 'rb').read() == open(out1 / f, 'rb').read(), f
    assert printed0 == printed1 and 'boundary' not in printed0 and set(stats0) == {'segm', 'bbox'}
    out2, stats2 = _evaluate(tmp_path, 'on', ['--boundary', '1'])
    printed2 = capsys.readouterr().out
    metrics = json.load(open(out2 / 'metrics.json'))
    assert metrics == stats2 and set(metrics) == {'segm', 'bbox', 'boundary'} and len(metrics['boundary']) == 12
    assert metrics['segm'] == stats0['segm'] and metrics['bbox'] == stats0['bbox']
    assert printed2.startswith(printed0) and 'iouType: boundary' in printed2[len(printed0):]
    for f in files[:2]:
        assert open(out0 / f, 'rb').read() == open(out2 / f, 'rb').read(), f
    assert len(json.load(open(out2 / 'segm_results.json'))) > 0


def _train_args(out, extra):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', '4', '--batch-size', '1', '--image-size', '256', '320',
                                            '--log-interval', '2', '--snapshot-interval', '4', '--label_file', '/nonexistent'] + extra)


def test_train_eval_boundary_logs_keys_and_does_not_perturb_training(tmp_path):
    import train
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    train.run(_train_args(a, ['--eval-interval', '2', '--eval-images', '2', '--eval-metric', 'mask_coco', '--eval-boundary', '1']))
    train.run(_train_args(b, []))
    la = [json.loads(l) for l in open(os.path.join(a, 'log'))]
    lb = [json.loads(l) for l in open(os.path.join(b, 'log'))]
    assert [e['iteration'] for e in la] == [2, 4] == [e['iteration'] for e in lb]
    keys = ['validation/main/%s' % k for k in ('map', 'ap50', 'ap75', 'ap_small', 'ap_medium', 'ap_large', 'ar')]
    for e in la:
        for k in keys + [k.replace('main/', 'main/bbox/') for k in keys] + [k.replace('main/', 'main/boundary/') for k in keys]:
            assert k in e and (e[k] == -1.0 or 0.0 <= e[k] <= 1.0), (k, e.get(k))
    assert not any(k.startswith('validation/') for e in lb for k in e)
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    for x, y in zip(la, lb):
        assert x['main/loss'] == y['main/loss']
