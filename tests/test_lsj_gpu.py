"""GPU tests of large-scale jitter (csrc/augment.hip crop kernels, dataset/loader.py, train.py --lsj-size): the image
writer bit-exactly against the sliced NumPy resize and against the shipped batched kernel, the box / compaction kernels and the gathering
mask writer against NumPy on constructed masks, the device loader against the host transforms on the same decisions, and a training run
with large-scale jitter that resumes bit-identically."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.dataset import augment  # noqa: E402
from chainer_maskrcnn.dataset.augment import Augment, lsj_geometry  # noqa: E402
from chainer_maskrcnn.dataset.loader import BatchLoader  # noqa: E402
from chainer_maskrcnn.dataset.transforms import KeypointTransform, RawTransform, Transform, resize_linear  # noqa: E402
from tests.augment_data import write_coco  # noqa: E402
from tests.augment_edge_cases import np_crop as _np_crop  # noqa: E402  (the NumPy rule, shared with tests/test_augment_edges_gpu.py)

DEV = 'cuda:0'
CANVASES = [(64, 64), (61, 50)]          # the second: a ragged row (dst_w % 4 != 0, % 16 != 0) takes the scalar stores


def _packed(arrays):
    offs = np.cumsum([0] + [a.nbytes for a in arrays])
    buf = np.concatenate([a.reshape(-1) for a in arrays]) if arrays else np.zeros((0,), np.uint8)
    return torch.from_numpy(buf).to(DEV), [int(o) for o in offs[:-1]]


def _fit(geo, canvas):
    """(oh, ow, y0, x0, ch, cw) with the window cut to the canvas (the ragged canvas is smaller than the S = 64 the geometry was made for)."""
    oh, ow, y0, x0, ch, cw = geo
    return oh, ow, y0, x0, min(ch, canvas[0]), min(cw, canvas[1])


# (H, W, flip, geometry): upscaled 2x with an interior window, mirrored; downscaled to 0.1, far smaller than the canvas; scale 1 (the
# virtual resize is the source itself) wider than the canvas and lower; s = 1.37 of a wide source through lsj_geometry
IMAGE_CASES = [(40, 52, 1, lsj_geometry(40, 52, 64, 2.0, 0.5, 0.5)), (91, 127, 0, lsj_geometry(91, 127, 64, 0.1, 0.7, 0.2)),
               (50, 90, 0, (50, 90, 0, 13, 50, 64)), (37, 100, 1, lsj_geometry(37, 100, 64, 1.37, 0.3, 0.999999))]


def test_image_cases_are_what_they_claim():
    (oh, ow, y0, x0, ch, cw) = IMAGE_CASES[0][3]
    assert ow == 128 and 0 < y0 < oh - ch and 0 < x0 < ow - cw and (ch, cw) == (64, 64)
    assert IMAGE_CASES[1][3] == (5, 6, 0, 0, 5, 6)
    assert IMAGE_CASES[3][3][1] > 64 > IMAGE_CASES[3][3][0] and IMAGE_CASES[3][3][3] == IMAGE_CASES[3][3][1] - 64


@pytest.mark.parametrize('canvas', CANVASES, ids=['64x64', 'ragged_61x50'])
def test_image_crop_writer_equals_the_sliced_resize(canvas):
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W, _, _ in IMAGE_CASES]
    src, offs = _packed(imgs)
    geos = [_fit(c[3], canvas) for c in IMAGE_CASES]
    desc = ops.crop_descs([(o, H, W, g[0], g[1], flip, 0) + g[2:] for o, (H, W, flip, _), g in zip(offs, IMAGE_CASES, geos)])
    out = ops.image_resize_crop_batch_u8(src, desc, canvas[0], canvas[1], 255.0).cpu().numpy()
    want = np.zeros((len(imgs), 3) + canvas, np.float32)
    for n, (img, (H, W, flip, _), (oh, ow, y0, x0, ch, cw)) in enumerate(zip(imgs, IMAGE_CASES, geos)):
        chw = img.transpose(2, 0, 1).astype(np.float32)
        want[n, :, :ch, :cw] = (resize_linear(chw[..., ::-1] if flip else chw, (oh, ow)) / np.float32(255))[:, y0:y0 + ch, x0:x0 + cw]
    np.testing.assert_array_equal(out, want)
    assert np.count_nonzero(out[1, :, 5:]) == 0 and np.count_nonzero(out[1, :, :, 6:]) == 0 and np.count_nonzero(out[1]) > 0
    # the shipped batched kernel at (oh, ow), sliced: the second oracle
    Hp, Wp = max(g[0] for g in geos), max(g[1] for g in geos)
    full = ops.image_resize_batch_u8(src, ops.resize_descs([(o, H, W, g[0], g[1], flip, 0) for o, (H, W, flip, _), g in
                                                            zip(offs, IMAGE_CASES, geos)]), Hp, Wp, 255.0).cpu().numpy()
    for n, (oh, ow, y0, x0, ch, cw) in enumerate(geos):
        np.testing.assert_array_equal(out[n, :, :ch, :cw], full[n, :, y0:y0 + ch, x0:x0 + cw])


# ---- boxes, compaction and the gathering mask writer -------------------------------------------------------------------------------
def _rect(H, W, ys, xs):
    m = np.zeros((H, W), np.uint8)
    m[ys[0]:ys[1], xs[0]:xs[1]] = 1
    return m


def _mask_batch(flip, canvas):
    """Four examples as the kernels see them: (masks (count,H,W), flip, geometry).  The constructed layouts are what the crop sees, so for
    flip = 1 the sources are stored mirrored."""
    rs = np.random.RandomState(4)
    H, W = 80, 90                                            # scale 1: the 64 x 64 window at (10, 20) of the source itself
    a = [_rect(H, W, (20, 30), (30, 40)),                    # inside
         _rect(H, W, (0, 15), (40, 50)),                     # cut at the top
         _rect(H, W, (70, 80), (40, 50)),                    # cut at the bottom
         _rect(H, W, (0, 5), (0, 10)),                       # outside: dropped from the middle of the list
         _rect(H, W, (30, 40), (10, 25)),                    # cut at the left
         _rect(H, W, (30, 40), (80, 90)),                    # cut at the right
         _rect(H, W, (73, 80), (83, 90))]                    # one pixel survives, at the window's corner
    b = [_rect(60, 60, (0, 6), (0, 6)), _rect(60, 60, (50, 60), (50, 60))]      # upscaled 2x, the window in the middle: both outside
    c = [(rs.rand(33, 47) > 0.97).astype(np.uint8), _rect(33, 47, (2, 4), (40, 44)), (rs.rand(33, 47) > 0.5).astype(np.uint8)]
    exs = [(np.stack(a), (80, 90, 10, 20, 64, 64)), (np.stack(b), (120, 120, 28, 28, 64, 64)),
           (np.stack(c), lsj_geometry(33, 47, 64, 1.7, 0.6, 0.3)), (np.zeros((0, 20, 30), np.uint8), lsj_geometry(20, 30, 64, 0.5, 0.0, 0.0))]
    return [(np.ascontiguousarray(m[:, :, ::-1]) if flip else m, flip, _fit(g, canvas)) for m, g in exs]


def _run_boxes(batch, G, canvas):
    Gin = max(1, max(m.shape[0] for m, _, _ in batch))
    labels_in = np.full((len(batch), Gin), -1, np.int32)
    for n, (m, _, _) in enumerate(batch):
        labels_in[n, :m.shape[0]] = 10 * (n + 1) + np.arange(m.shape[0])
    src, offs = _packed([m for m, _, _ in batch])
    desc = ops.crop_descs([(o, m.shape[1], m.shape[2], g[0], g[1], flip, m.shape[0]) + g[2:] for o, (m, flip, g) in zip(offs, batch)])
    got = ops.mask_crop_boxes_u8(src, desc, torch.from_numpy(labels_in).to(DEV), G, canvas[0], canvas[1])
    return src, desc, labels_in, got


@pytest.mark.parametrize('flip', [0, 1], ids=['unflipped', 'flipped'])
def test_crop_boxes_and_compaction_equal_numpy(flip):
    canvas = (64, 64)
    batch = _mask_batch(flip, canvas)
    for G in (3, 7):                                         # 3: kept instances past the last output row are dropped
        _, _, labels_in, (bboxes, labels, gather) = _run_boxes(batch, G, canvas)
        wb, wl, wg, _ = _np_crop(batch, labels_in, G)
        np.testing.assert_array_equal(gather.cpu().numpy(), wg)
        np.testing.assert_array_equal(labels.cpu().numpy(), wl)
        np.testing.assert_array_equal(bboxes.cpu().numpy(), wb)
        assert bboxes.dtype == torch.float32 and labels.dtype == torch.int32 and gather.dtype == torch.int32
    # the constructed cases are what they claim (G = 7)
    assert wg[0].tolist() == [0, 1, 2, 4, 5, 6, -1] and wl[0].tolist() == [10, 11, 12, 14, 15, 16, -1]
    np.testing.assert_array_equal(wb[0], [[10, 10, 20, 20], [0, 20, 5, 30], [60, 20, 64, 30], [20, 0, 30, 5], [20, 60, 30, 64],
                                          [63, 63, 64, 64], [0, 0, 0, 0]])
    assert wl[1].tolist() == [-1] * 7 and not wb[1].any() and wg[1].tolist() == [-1] * 7          # every instance dropped
    assert 0 < (wl[2] >= 0).sum() <= 3 and wl[2, 3:].tolist() == [-1] * 4                       # a count below G
    assert wl[3].tolist() == [-1] * 7                                                           # count 0


@pytest.mark.parametrize('canvas', CANVASES, ids=['64x64', 'ragged_61x50'])
@pytest.mark.parametrize('flip', [0, 1], ids=['unflipped', 'flipped'])
def test_mask_crop_writer_gathers_the_kept_planes(flip, canvas):
    batch = _mask_batch(flip, canvas)
    G = 7
    src, desc, labels_in, (bboxes, labels, gather) = _run_boxes(batch, G, canvas)
    out = ops.mask_resize_crop_batch_u8(src, desc, gather, canvas[0], canvas[1]).cpu().numpy()
    wb, wl, wg, planes = _np_crop(batch, labels_in, G)
    np.testing.assert_array_equal(gather.cpu().numpy(), wg)
    np.testing.assert_array_equal(bboxes.cpu().numpy(), wb)
    want = np.zeros((len(batch), G) + canvas, np.uint8)
    for n, (ps, kept) in enumerate(planes):
        for j, g in enumerate(kept):
            want[n, j, :ps[g].shape[0], :ps[g].shape[1]] = ps[g]
    np.testing.assert_array_equal(out, want)
    assert not out[1].any() and not out[3].any()
    if canvas == (64, 64):
        assert out[0, :6].reshape(6, -1).any(1).all() and not out[0, 6:].any()
    # any table works: -1 in the middle and entries outside the example's count are zero planes, an instance may be read twice
    table = np.array([[6, -1, 0, 0, 7, 100, 3], [1, 0, -1, -1, -1, -1, -1], [2, 2, 1, 0, 3, -1, -1], [0, -1, -1, -1, -1, -1, -1]], np.int32)
    out = ops.mask_resize_crop_batch_u8(src, desc, torch.from_numpy(table).to(DEV), canvas[0], canvas[1]).cpu().numpy()
    want[:] = 0
    for n, (ps, _) in enumerate(planes):
        for j, g in enumerate(table[n]):
            if 0 <= g < len(ps):
                want[n, j, :ps[g].shape[0], :ps[g].shape[1]] = ps[g]
    np.testing.assert_array_equal(out, want)


# ---- the device loader against the host transforms ----------------------------------------------------------------------------------
class _Sizes(object):
    min_size, max_size = 96, 160


def _loaders(ds, host_tf, dev_tf, aug, keypoints=False, max_gt=3):
    kw = dict(batch_size=2, shuffle=True, seed=2, num_workers=2, max_gt=max_gt, keypoints=keypoints, device=DEV, augment=aug)
    return BatchLoader(ds, host_tf, **kw), BatchLoader(ds, dev_tf, **kw)


def _compare(host, devl, n, keys, max_gt=3):
    try:
        for _ in range(n):
            a, b = next(host), next(devl)
            for k in keys:
                x, y = a[k], b[k]
                x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
                y = y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
                if max_gt is None and k in ('masks', 'bboxes', 'labels') and y.shape[1] > x.shape[1]:
                    # without max_gt the device path sizes G by the instances BEFORE the crop (it does not wait for the kept count);
                    # the host collates the kept ones: the device's extra rows are empty
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
def test_lsj_device_loader_equals_host_transform(tmp_path, max_gt):
    from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader
    root = write_coco(str(tmp_path), n_img=5, sizes=[(97, 131), (120, 100), (91, 157), (128, 128), (101, 99)])
    ds = COCOMaskLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    aug = Augment(hflip_prob=0.5, seed=9, lsj_size=64)
    drawn = [aug.params(0, t) for t in range(12)]
    assert any(p.flip for p in drawn) and not all(p.flip for p in drawn)
    assert min(p.lsj[1] for p in drawn) < 0.6 and max(p.lsj[1] for p in drawn) > 1.4
    host, devl = _loaders(ds, Transform(_Sizes()), RawTransform(_Sizes()), aug, max_gt=max_gt)
    _compare(host, devl, 6, ('imgs', 'masks', 'bboxes', 'labels', 'scales', 'sizes'), max_gt)


def test_lsj_device_loader_equals_host_transform_keypoints(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOKeypointsLoader
    root = write_coco(str(tmp_path), n_img=5, sizes=[(97, 131), (120, 100), (91, 157), (128, 128), (101, 99)])
    ds = COCOKeypointsLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    perm = augment.flip_permutation(ds.coco.cats[1]['keypoints'])
    aug = Augment(hflip_prob=0.5, seed=9, keypoint_perm=perm, lsj_size=64)
    host, devl = _loaders(ds, KeypointTransform(_Sizes()), RawTransform(_Sizes(), keypoints=True), aug, keypoints=True)
    _compare(host, devl, 6, ('imgs', 'keypoints', 'bboxes', 'labels', 'scales', 'sizes'))


# ---- training -----------------------------------------------------------------------------------------------------------------------
def _train_args(out, root, iteration, extra=(), resume=''):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', str(iteration), '--batch-size', '2', '--synthetic', '0',
                                            '--anno-dir', root + '/annotations', '--img-dir', root, '--num-workers', '2',
                                            '--log-interval', '2', '--snapshot-interval', '2', '--label_file', '/nonexistent']
                                           + list(extra) + (['--resume', resume] if resume else []))


def test_lsj_training_resumes_bit_identically(tmp_path):
    import json
    import train
    root = write_coco(str(tmp_path / 'data'), n_img=6)
    aug = ['--lsj-size', '64', '--hflip', '1']
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    train.run(_train_args(a, root, 4, aug))
    ck = os.path.join(a, 'trainer_2.pt')
    assert torch.load(ck, weights_only=False)['augment'] == {'hflip': 1, 'min_sizes': None, 'seed': train.AUGMENT_SEED,
                                                             'lsj': {'size': 64, 'scale': [0.1, 2.0]}}
    train.run(_train_args(b, root, 4, aug, resume=ck))
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    for out in (a, b):
        log = [json.loads(l) for l in open(os.path.join(out, 'log'))]
        assert log[-1]['iteration'] == 4 and all(np.isfinite(v) for e in log for k, v in e.items() if k.startswith('main/'))
    with pytest.raises(ValueError, match='augmentation'):
        train.run(_train_args(str(tmp_path / 'c'), root, 4, aug + ['--lsj-scale', '0.5', '2.0'], resume=ck))
