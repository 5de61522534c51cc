"""GPU tests of the training augmentation (csrc/augment.hip, dataset/loader.py, train.py --hflip / --min-sizes): the
batched resize kernels bit-exactly against the NumPy restatement of the mirrored resize and against the per-image kernels, the
augmented device loader against the host Transform on the same decisions, and an augmented training run that resumes bit-identically."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn._hip import check, lib, ops, ptr  # noqa: E402
from chainer_maskrcnn.dataset import augment  # noqa: E402
from chainer_maskrcnn.dataset.augment import Augment  # noqa: E402
from chainer_maskrcnn.dataset.loader import BatchLoader  # noqa: E402
from chainer_maskrcnn.dataset.transforms import KeypointTransform, RawTransform, Transform, resize_linear, resize_nearest  # noqa: E402
from tests.augment_data import write_coco  # noqa: E402

DEV = 'cuda:0'

# (H, W, oh, ow, flip): odd and even widths, down- and upscaling, oh, ow == H, W
IMAGE_CASES = [(37, 51, 20, 33, 1), (64, 48, 64, 48, 1), (30, 41, 75, 97, 1), (50, 64, 50, 64, 0), (33, 20, 71, 40, 0),
               (91, 127, 61, 85, 1)]


def _packed(arrays):
    offs = np.cumsum([0] + [a.nbytes for a in arrays])
    buf = np.concatenate([a.reshape(-1) for a in arrays]) if arrays else np.zeros((0,), np.uint8)
    return torch.from_numpy(buf).to(DEV), [int(o) for o in offs[:-1]]


def _images(rs, cases):
    return [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W, _, _, _ in cases]


@pytest.mark.parametrize('pad', [(0, 0), (5, 3)], ids=['pad64', 'ragged_row'])
def test_batched_image_resize_equals_numpy_flip(pad):
    rs = np.random.RandomState(0)
    imgs = _images(rs, IMAGE_CASES)
    src, offs = _packed(imgs)
    desc = ops.resize_descs([(o,) + c[:4] + (c[4], 0) for o, c in zip(offs, IMAGE_CASES)])
    Hp = -(-max(c[2] for c in IMAGE_CASES) // 64) * 64 + pad[0]
    Wp = -(-max(c[3] for c in IMAGE_CASES) // 64) * 64 + pad[1]          # (ragged: rows of Wp % 4 != 0 take the scalar stores)
    out = ops.image_resize_batch_u8(src, desc, Hp, Wp, 255.0).cpu().numpy()
    want = np.zeros((len(imgs), 3, Hp, Wp), np.float32)
    for n, (img, (H, W, oh, ow, flip)) in enumerate(zip(imgs, IMAGE_CASES)):
        chw = img.transpose(2, 0, 1).astype(np.float32)
        want[n, :, :oh, :ow] = resize_linear(chw[..., ::-1] if flip else chw, (oh, ow)) / np.float32(255)
    np.testing.assert_array_equal(out, want)
    assert np.count_nonzero(out[0, :, IMAGE_CASES[0][2]:, :]) == 0 and np.count_nonzero(out[0, :, :, IMAGE_CASES[0][3]:]) == 0


@pytest.mark.parametrize('pad', [(0, 0), (3, 7)], ids=['pad64', 'ragged_row'])
def test_batched_mask_resize_equals_numpy_flip(pad):
    rs = np.random.RandomState(1)
    counts = [2, 0, 3, 1, 4, 1]
    G = 4
    masks = [(rs.rand(g, H, W) > 0.5).astype(np.uint8) for g, (H, W, _, _, _) in zip(counts, IMAGE_CASES)]
    src, offs = _packed(masks)
    desc = ops.resize_descs([(o,) + c[:4] + (c[4], g) for o, c, g in zip(offs, IMAGE_CASES, counts)])
    Hp = -(-max(c[2] for c in IMAGE_CASES) // 64) * 64 + pad[0]
    Wp = -(-max(c[3] for c in IMAGE_CASES) // 64) * 64 + pad[1]
    out = ops.mask_resize_batch_u8(src, desc, G, Hp, Wp).cpu().numpy()
    want = np.zeros((len(masks), G, Hp, Wp), np.uint8)
    for n, (m, (H, W, oh, ow, flip), g) in enumerate(zip(masks, IMAGE_CASES, counts)):
        for k in range(g):
            want[n, k, :oh, :ow] = resize_nearest(m[k][:, ::-1] if flip else m[k], (oh, ow))
    np.testing.assert_array_equal(out, want)
    empty, _ = _packed([np.zeros((0, 5, 5), np.uint8)])                  # no instance in the whole batch: all zero, no source read
    z = ops.mask_resize_batch_u8(empty, ops.resize_descs([(0, 5, 5, 7, 9, 1, 0)]), 2, 64, 64)
    assert z.shape == (1, 2, 64, 64) and int(z.count_nonzero()) == 0


def test_batched_kernels_without_flip_equal_the_per_image_kernels():
    rs = np.random.RandomState(2)
    cases = [c[:4] + (0,) for c in IMAGE_CASES]
    imgs = _images(rs, cases)
    counts = [1, 3, 2, 0, 2, 1]
    G = 3
    masks = [(rs.rand(g, H, W) > 0.3).astype(np.uint8) for g, (H, W, _, _, _) in zip(counts, cases)]
    Hp, Wp = 128, 128
    src, offs = _packed(imgs)
    got = ops.image_resize_batch_u8(src, ops.resize_descs([(o,) + c + (0,) for o, c in zip(offs, cases)]), Hp, Wp, 255.0)
    msrc, moffs = _packed(masks)
    gotm = ops.mask_resize_batch_u8(msrc, ops.resize_descs([(o,) + c + (g,) for o, c, g in zip(moffs, cases, counts)]), G, Hp, Wp)
    want = torch.zeros((len(imgs), 3, Hp, Wp), dtype=torch.float32, device=DEV)
    wantm = torch.zeros((len(imgs), G, Hp, Wp), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    for n, (img, m, (H, W, oh, ow, _), g) in enumerate(zip(imgs, masks, cases, counts)):
        raw = torch.from_numpy(img).to(DEV)
        check(lib().mrcnn_image_resize_u8_f32(ptr(raw), H, W, ptr(want[n]), oh, ow, Hp, Wp, 255.0, st))
        if g:
            mr = torch.from_numpy(m).to(DEV)
            check(lib().mrcnn_mask_resize_nearest_u8(ptr(mr), g, H, W, ptr(wantm[n]), oh, ow, Hp, Wp, st))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(gotm, wantm)


def test_batched_kernels_refuse_bad_arguments():
    src, offs = _packed([np.zeros((4, 6, 3), np.uint8)])
    out = torch.empty((1, 3, 8, 8), dtype=torch.float32, device=DEV)
    stp = torch.cuda.current_stream().cuda_stream
    for row in [(0, 4, 6, 9, 6, 0, 0), (0, 4, 6, 8, 8, 2, 0), (1, 4, 6, 8, 8, 0, 0), (0, 0, 6, 8, 8, 0, 0)]:
        d = ops.resize_descs([row])
        assert lib().mrcnn_image_resize_batch_u8_f32(ptr(src), src.numel(), d.ctypes.data, 1, ptr(out), 8, 8, 255.0, stp) == -1
    d = ops.resize_descs([(0, 4, 6, 8, 8, 0, 0)])
    assert lib().mrcnn_image_resize_batch_u8_f32(ptr(src), src.numel(), d.ctypes.data, 0, ptr(out), 8, 8, 255.0, stp) == -1
    m = torch.empty((1, 1, 8, 8), dtype=torch.uint8, device=DEV)
    d = ops.resize_descs([(0, 4, 6, 8, 8, 0, 2)])                        # count > G
    assert lib().mrcnn_mask_resize_batch_nearest_u8(ptr(src), src.numel(), d.ctypes.data, 1, 1, ptr(m), 8, 8, stp) == -1


class _Sizes(object):
    min_size, max_size = 96, 160


def _loaders(ds, host_tf, dev_tf, aug, keypoints=False):
    kw = dict(batch_size=2, shuffle=True, seed=2, num_workers=2, max_gt=3, keypoints=keypoints, device=DEV, augment=aug)
    return BatchLoader(ds, host_tf, **kw), BatchLoader(ds, dev_tf, **kw)


def _compare(host, devl, n, keys):
    try:
        for _ in range(n):
            a, b = next(host), next(devl)
            for k in keys:
                x, y = a[k], b[k]
                x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
                y = y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
                np.testing.assert_array_equal(x, y, err_msg=k)
    finally:
        host.close()
        devl.close()


def test_augmented_device_loader_equals_host_transform(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader
    root = write_coco(str(tmp_path), n_img=5, sizes=[(97, 131), (120, 100), (91, 157), (128, 128), (101, 99)])
    ds = COCOMaskLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    aug = Augment(hflip_prob=0.5, min_sizes=[80, 112, 144], seed=9)
    drawn = [aug.params(0, t) for t in range(8)]
    assert any(p.flip for p in drawn) and not all(p.flip for p in drawn) and len({p.min_size for p in drawn}) > 1
    host, devl = _loaders(ds, Transform(_Sizes()), RawTransform(_Sizes()), aug)
    _compare(host, devl, 4, ('imgs', 'masks', 'bboxes', 'labels', 'scales', 'sizes'))


def test_augmented_device_loader_equals_host_transform_keypoints(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOKeypointsLoader
    root = write_coco(str(tmp_path), n_img=5, sizes=[(97, 131), (120, 100), (91, 157), (128, 128), (101, 99)])
    ds = COCOKeypointsLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    perm = augment.flip_permutation(ds.coco.cats[1]['keypoints'])
    aug = Augment(hflip_prob=0.5, min_sizes=[80, 112, 144], seed=9, keypoint_perm=perm)
    host, devl = _loaders(ds, KeypointTransform(_Sizes()), RawTransform(_Sizes(), keypoints=True), aug, keypoints=True)
    _compare(host, devl, 4, ('imgs', 'keypoints', 'bboxes', 'labels', 'scales', 'sizes'))


def _train_args(out, root, iteration, extra=(), resume=''):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', str(iteration), '--batch-size', '2', '--synthetic', '0',
                                            '--anno-dir', root + '/annotations', '--img-dir', root, '--num-workers', '2',
                                            '--log-interval', '2', '--snapshot-interval', '2', '--label_file', '/nonexistent']
                                           + list(extra) + (['--resume', resume] if resume else []))


def test_augmented_training_resumes_bit_identically(tmp_path):
    import json
    import train
    root = write_coco(str(tmp_path / 'data'), n_img=6)
    aug = ['--hflip', '1', '--min-sizes', '96', '128']
    a, b, c = str(tmp_path / 'a'), str(tmp_path / 'b'), str(tmp_path / 'c')
    train.run(_train_args(a, root, 4, aug))
    assert torch.load(os.path.join(a, 'trainer_2.pt'), weights_only=False)['augment'] == {'hflip': 1, 'min_sizes': [96, 128],
                                                                                          'seed': train.AUGMENT_SEED}
    train.run(_train_args(b, root, 4, aug, resume=os.path.join(a, 'trainer_2.pt')))
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    for out in (a, b):
        log = [json.loads(l) for l in open(os.path.join(out, 'log'))]
        assert log[-1]['iteration'] == 4 and all(np.isfinite(v) for e in log for k, v in e.items() if k.startswith('main/'))
    train.run(_train_args(c, root, 4))                                   # the same run without augmentation
    zc = np.load(os.path.join(c, 'model_4.npz'))
    assert not np.array_equal(za['head/fc2/W'], zc['head/fc2/W'])
