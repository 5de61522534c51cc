"""GPU tests of Simple Copy-Paste (csrc/copy_paste.hip, ops.copy_paste, dataset/loader.py, train.py --copy-paste): the
kernels bit for bit against the NumPy rule (dataset/augment.py copy_paste_batch, itself pinned to literal labels and boxes by
tests/test_copy_paste_cpu.py) on a hand-made batch, the offer looked up through the gather table, the device loader against the host loader
on the same decisions, and a training run with Copy-Paste that resumes bit-identically.  The rule has no rounding: every comparison is
exact."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.dataset.augment import Augment, copy_paste_batch  # noqa: E402
from chainer_maskrcnn.dataset.loader import BatchLoader, collate  # noqa: E402
from chainer_maskrcnn.dataset.transforms import RawTransform, Transform  # noqa: E402
from tests.augment_data import write_coco  # noqa: E402
from tests.copy_paste_data import CANVASES, handmade, offers_of  # noqa: E402

DEV = 'cuda:0'


def _device(batch, gather, sel, receive, G_out):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    given = [t(batch['imgs']), t(batch['masks']), t(batch['labels']), t(gather), t(sel), t(receive)]
    before = [g.clone() for g in given]
    imgs, masks, bboxes, labels = ops.copy_paste(*given, G_out)
    for g, b in zip(given, before):                          # the pre-paste batch is only read
        assert torch.equal(g, b)
    assert imgs.dtype == torch.float32 and masks.dtype == torch.uint8 and bboxes.dtype == torch.float32 and labels.dtype == torch.int32
    return {'imgs': imgs.cpu().numpy(), 'masks': masks.cpu().numpy(), 'bboxes': bboxes.cpu().numpy(), 'labels': labels.cpu().numpy()}


def _check(got, want):
    for k in ('labels', 'bboxes', 'masks', 'imgs'):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize('canvas', CANVASES, ids=['64x64', 'ragged_61x50'])
def test_the_hand_made_batch_is_what_it_claims(canvas):
    H, W = canvas
    batch, gather, sel, receive = handmade(canvas)
    offers = offers_of(gather, sel)
    out = copy_paste_batch(batch, receive, offers, 4)
    m, lab = batch['masks'], batch['labels']
    alpha0 = (m[1, 0] | m[1, 1]).astype(bool)
    assert m[0, 0].any() and not (m[0, 0] * ~alpha0).any() and 1 not in out['labels'][0]                 # a dropped instance
    assert (m[0, 1] * alpha0).any() and (m[0, 1] * ~alpha0).any()                                        # a cut one: its box shrinks
    assert batch['bboxes'][0, 1].tolist() == [30, 30, 40, 40] and out['bboxes'][0, 0].tolist() == [30, 30, 35, 40]
    assert lab[1, 2] == 5 and not offers[1][2] and 5 not in out['labels'][0] and not (m[1, 2] * alpha0).any()   # a valid row that is not offered
    assert lab[0, 2] == -1 and sel[0, 2] == 1 and gather[0, 2] == -1                                     # an empty row is never a source
    assert receive[1] and not any(offers[2]) and out['labels'][1].tolist() == [3, 4, 5, -1]              # an empty offer
    assert not receive[2] and all(offers[0][:2]) and out['labels'][2].tolist() == [6, -1, -1, -1]        # receive = 0 against a full offer
    assert out['labels'][0].tolist() == [2, 3, 4, -1]
    assert copy_paste_batch(batch, receive, offers, 2)['labels'].tolist() == [[2, 3], [3, 4], [6, -1]]   # truncation
    edges = [4, 20, 30, 40, 0, 26, 20, 46, 33]               # first and one-past-last columns of the rectangles
    assert sum(e % 16 != 0 for e in edges) >= 7                                                          # off the 16-byte thread boundary
    assert m[2, 0][:, W - 1].any() and m[1, 2][H - 1, W - 1]                                             # masks touching the last column
    assert (W % 16 != 0) == (canvas == (61, 50)) and len(set((np.asarray(gather) >= 0).sum(1))) == 3
    assert (gather[lab >= 0] == np.nonzero(lab >= 0)[1]).all()                                           # gather = identity on valid rows


@pytest.mark.parametrize('G_out', [4, 2])
@pytest.mark.parametrize('canvas', CANVASES, ids=['64x64', 'ragged_61x50'])
def test_copy_paste_kernels_equal_the_numpy_rule(canvas, G_out):
    H, W = canvas
    batch, gather, sel, receive = handmade(canvas)
    want = copy_paste_batch(batch, receive, offers_of(gather, sel), G_out)
    got = _device(batch, gather, sel, receive, G_out)
    _check(got, want)
    # and the literal results
    assert got['labels'][0].tolist() == [2, 3, 4, -1][:G_out] and got['labels'][1].tolist() == [3, 4, 5, -1][:G_out]
    assert got['labels'][2].tolist() == [6, -1, -1, -1][:G_out]
    np.testing.assert_array_equal(got['bboxes'][0], np.array([[30, 30, 35, 40], [0, 0, 26, 26], [35, 20, 51, 46], [0, 0, 0, 0]], np.float32)[:G_out])
    alpha = (batch['masks'][1, 0] | batch['masks'][1, 1]).astype(bool)
    np.testing.assert_array_equal(got['imgs'][0] != batch['imgs'][0], np.broadcast_to(alpha, (3, H, W)))
    np.testing.assert_array_equal(got['imgs'][1:], batch['imgs'][1:])
    np.testing.assert_array_equal(got['masks'][1:, :min(G_out, 3)], batch['masks'][1:, :min(G_out, 3)])


def test_the_offer_is_looked_up_through_the_gather_table():
    """The rows as a crop leaves them: original instance 0 of every example was dropped, so row j holds original instance j + 1.  sel is
    keyed by the original index: example 1 offers originals 0 and 2 - its row 1, not its row 0 (whose original, 1, is not offered although
    the lower index 0 is); example 0 offers original 1, its row 0."""
    canvas = (61, 50)
    batch, _, _, _ = handmade(canvas)
    gather = np.array([[1, 2, -1], [1, 2, 3], [1, -1, -1]], np.int32)
    sel = np.array([[0, 1, 0, 0], [1, 0, 1, 0], [1, 1, 1, 1]], np.uint8)
    receive = np.array([1, 0, 1], np.uint8)
    offers = offers_of(gather, sel)
    assert [o.tolist() for o in offers] == [[True, False, False], [False, True, False], [True, False, False]]
    assert sel[1, gather[1, 0]] == 0 and sel[1, 0] == 1 and sel[1, gather[1, 1]] == 1
    want = copy_paste_batch(batch, receive, offers, 4)
    assert want['labels'].tolist() == [[1, 2, 4, -1], [3, 4, 5, -1], [6, 1, -1, -1]]
    np.testing.assert_array_equal(want['bboxes'][0, 1], [30, 30, 35, 40])
    _check(_device(batch, gather, sel, receive, 4), want)
    # a table entry outside sel's columns offers nothing, whatever sel holds
    gather[1, 1] = 4
    want = copy_paste_batch(batch, receive, offers_of(np.where(gather < 4, gather, -1), sel), 4)
    assert want['labels'][0].tolist() == [1, 2, -1, -1]
    _check(_device(batch, gather, sel, receive, 4), want)


# ---- the device loader against the host loader --------------------------------------------------------------------------------------
class _Sizes(object):
    min_size, max_size = 96, 160


SEED = 2            # chosen on the CPU, with the host rule: see the assertions in front of the comparison


def _compare(host, devl, n, keys, max_gt):
    try:
        for _ in range(n):
            a, b = next(host), next(devl)
            for k in keys:
                x, y = a[k], b[k]
                x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
                y = y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
                if max_gt is None and k in ('masks', 'bboxes', 'labels') and y.shape[1] > x.shape[1]:
                    # without max_gt the device path sizes its rows by the instances BEFORE the crop (it does not wait for the kept
                    # counts); the host sizes them by the kept ones: the device's extra rows are empty
                    g = x.shape[1]
                    assert (y[:, g:] == (-1 if k == 'labels' else 0)).all(), k
                    y = y[:, :g]
                assert x.dtype == y.dtype and x.shape == y.shape, k
                np.testing.assert_array_equal(x, y, err_msg=k)
            assert tuple(b['imgs'].shape[2:]) == (64, 64)
    finally:
        host.close()
        devl.close()


@pytest.mark.parametrize('max_gt', [3, 2, None])
def test_copy_paste_device_loader_equals_host_loader(tmp_path, max_gt):
    from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader
    root = write_coco(str(tmp_path), n_img=5, sizes=[(97, 131), (120, 100), (91, 157), (128, 128), (101, 99)])
    ds = COCOMaskLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    aug = Augment(hflip_prob=0.5, seed=SEED, lsj_size=64, copy_paste_prob=1.0)
    # what the 6 batches hold, by the host rule: at least one target instance covered entirely and dropped, and pasted instances
    tf = Transform(_Sizes())
    order = np.concatenate([np.random.RandomState(2 + e).permutation(len(ds)) for e in range(3)])
    dropped = pasted = 0
    for b in range(6):
        exs = [tf(ds[int(order[2 * b + j])], aug.params(0, 2 * b + j)) for j in range(2)]
        plain = collate([e[:5] for e in exs], max_gt, canvas=64)
        out = copy_paste_batch(plain, [e[5] for e in exs], [e[6] for e in exs], None)
        for n in range(2):
            assert exs[n][5] is True
            picked = int(np.asarray(exs[1 - n][6], bool)[:plain['labels'].shape[1]].sum())
            pasted += picked
            dropped += int((plain['labels'][n] >= 0).sum()) + picked - int((out['labels'][n] >= 0).sum())
    assert dropped >= 1 and pasted >= 1, (dropped, pasted)
    kw = dict(batch_size=2, shuffle=True, seed=2, num_workers=2, max_gt=max_gt, device=DEV, augment=aug)
    host, devl = BatchLoader(ds, tf, **kw), BatchLoader(ds, RawTransform(_Sizes()), **kw)
    _compare(host, devl, 6, ('imgs', 'masks', 'bboxes', 'labels', 'scales', 'sizes'), max_gt)


# ---- training -----------------------------------------------------------------------------------------------------------------------
def _train_args(out, root, iteration, extra=(), resume=''):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', str(iteration), '--batch-size', '2', '--synthetic', '0',
                                            '--anno-dir', root + '/annotations', '--img-dir', root, '--num-workers', '2',
                                            '--log-interval', '2', '--snapshot-interval', '2', '--label_file', '/nonexistent']
                                           + list(extra) + (['--resume', resume] if resume else []))


def test_copy_paste_training_resumes_bit_identically(tmp_path):
    import json
    import train
    root = write_coco(str(tmp_path / 'data'), n_img=6)
    aug = ['--lsj-size', '64', '--hflip', '1', '--copy-paste', '0.5']
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    train.run(_train_args(a, root, 4, aug))
    ck = os.path.join(a, 'trainer_2.pt')
    assert torch.load(ck, weights_only=False)['augment'] == {'hflip': 1, 'min_sizes': None, 'seed': train.AUGMENT_SEED,
                                                             'lsj': {'size': 64, 'scale': [0.1, 2.0]}, 'copy_paste': 0.5}
    train.run(_train_args(b, root, 4, aug, resume=ck))
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    for out in (a, b):
        log = [json.loads(l) for l in open(os.path.join(out, 'log'))]
        assert log[-1]['iteration'] == 4 and all(np.isfinite(v) for e in log for k, v in e.items() if k.startswith('main/'))
    with pytest.raises(ValueError, match='augmentation'):
        train.run(_train_args(str(tmp_path / 'c'), root, 4, ['--lsj-size', '64', '--hflip', '1', '--copy-paste', '0.25'], resume=ck))
