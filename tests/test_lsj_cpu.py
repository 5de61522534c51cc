"""CPU tests of large-scale jitter (dataset/augment.py decide_lsj / lsj_geometry, the host transforms, train.py --lsj-size / --lsj-scale;
DESIGN.md §3.17): the decisions and the geometry, the host Transform against the NumPy resizes and tight boxes, the keypoint rule, the
refusals and the resume record, and the crop entry points' argument checks, which need no device."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

from chainer_maskrcnn import _hip  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.dataset import augment  # noqa: E402
from chainer_maskrcnn.dataset.augment import Augment, AugmentParams, decide, decide_lsj, hflip, lsj_geometry  # noqa: E402
from chainer_maskrcnn.dataset.loader import BatchLoader, collate  # noqa: E402
from chainer_maskrcnn.dataset.transforms import (KeypointTransform, RawTransform, Transform, resize_bbox, resize_linear,  # noqa: E402
                                                 resize_nearest)
from tests.augment_data import write_coco  # noqa: E402


class _Sizes(object):
    min_size, max_size = 64, 100


# ---- decisions and geometry ---------------------------------------------------------------------------------------------------------
def test_decide_lsj_is_pure_and_flips_like_decide():
    for t in range(1000):
        got = decide_lsj(11, 1, t, 0.5, (0.1, 2.0))
        assert got == decide_lsj(11, 1, t, 0.5, (0.1, 2.0))
        assert got[0] == decide(11, 1, t, 0.5)[0]
        assert 0.1 <= got[1] <= 2.0 and 0.0 <= got[2] < 1.0 and 0.0 <= got[3] < 1.0
    draws = np.array([decide_lsj(11, 1, t, 0.5, (0.1, 2.0))[1:] for t in range(1000)])
    assert draws[:, 0].min() < 0.3 and draws[:, 0].max() > 1.8 and len(set(draws[:, 1])) == 1000
    assert decide_lsj(11, 0, 3, 0.5, (0.1, 2.0)) != decide_lsj(11, 1, 3, 0.5, (0.1, 2.0))       # ranks draw their own
    assert decide_lsj(7, 0, 3, 0.5, (0.8, 0.8))[1] == 0.8
    assert decide(11, 1, 5, 0.5, [600, 800]) == (decide(11, 1, 5, 0.5)[0], decide(11, 1, 5, 0.5, [600, 800])[1])     # decide is unchanged


def test_lsj_geometry_keeps_the_window_inside_the_virtual_resize():
    us = (0.0, 0.5, 0.999999)
    for H, W, S, s in itertools.product((37, 64, 100, 480), (37, 64, 100, 480), (64, 128), (0.1, 0.5, 1, 1.37, 2)):
        r = min(S * s / H, S * s / W)
        for u_y, u_x in itertools.product(us, us):
            oh, ow, y0, x0, ch, cw = lsj_geometry(H, W, S, s, u_y, u_x)
            assert (oh, ow) == (max(1, int(H * r + 0.5)), max(1, int(W * r + 0.5)))
            assert (ch, cw) == (min(oh, S), min(ow, S))
            assert 0 <= y0 and y0 + ch <= oh and 0 <= x0 and x0 + cw <= ow
            assert (y0, x0) == (int(u_y * (oh - ch + 1)), int(u_x * (ow - cw + 1)))
            if oh <= S:
                assert y0 == 0
            if ow <= S:
                assert x0 == 0
            if u_y == 0.999999:
                assert y0 == oh - ch                                 # the last position is reachable
    assert lsj_geometry(480, 480, 64, 2, 0.5, 0.5) == (128, 128, 32, 32, 64, 64)
    assert lsj_geometry(100, 480, 64, 0.1, 0.9, 0.9) == (1, 6, 0, 0, 1, 6)


def test_augment_params_and_augment_keep_their_old_forms():
    p = AugmentParams(True, 48)
    assert p.keypoint_perm is None and p.lsj is None and AugmentParams(False, None, [1, 0]).lsj is None
    a = Augment(hflip_prob=0.5, min_sizes=[64, 80], seed=3)
    assert a.lsj_size is None and a.params(0, 4) == AugmentParams(*decide(3, 0, 4, 0.5, [64, 80]), None)
    b = Augment(hflip_prob=0.5, seed=3, lsj_size=128, lsj_scale=(0.5, 1.5))
    flip, s, u_y, u_x = decide_lsj(3, 2, 9, 0.5, (0.5, 1.5))
    assert b.params(2, 9) == AugmentParams(flip, None, None, (128, s, u_y, u_x))
    for bad in (dict(lsj_size=100), dict(lsj_size=-64), dict(lsj_size=64, lsj_scale=(0.0, 1.0)), dict(lsj_size=64, lsj_scale=(1.5, 1.0)),
                dict(lsj_size=64, min_sizes=[600])):
        with pytest.raises(ValueError):
            Augment(**bad)


# ---- host Transform -----------------------------------------------------------------------------------------------------------------
def _np_tight(m):
    ys, xs = np.nonzero(m)
    return [ys.min(), xs.min(), ys.max() + 1, xs.max() + 1] if len(ys) else None


def test_host_transform_with_lsj_is_the_sliced_resize_of_the_flipped_example():
    rs = np.random.RandomState(0)
    H, W, G = 37, 51, 4
    img = rs.randint(0, 256, (3, H, W)).astype(np.float32)
    masks = [(rs.rand(H, W) > 0.6).astype(np.uint8) for _ in range(G)]
    masks[2][:] = 0
    masks[2][3:6, 2:5] = 1                                   # a small instance: outside most windows
    ex = (img, rs.rand(G, 4).astype(np.float32) * 30, np.arange(G, dtype=np.int32) + 5, masks)
    dropped = 0
    for flip, S, s, u_y, u_x in ((True, 64, 2.0, 0.5, 0.5), (False, 64, 2.0, 0.999999, 0.0), (True, 64, 0.1, 0.3, 0.7), (False, 64, 1.0, 0.2, 0.9),
                                 (True, 128, 1.37, 0.0, 0.999999)):
        got = Transform(_Sizes())(ex, AugmentParams(flip, None, None, (S, s, u_y, u_x)))
        src = hflip(ex) if flip else ex
        oh, ow, y0, x0, ch, cw = lsj_geometry(H, W, S, s, u_y, u_x)
        np.testing.assert_array_equal(got[0], (resize_linear(src[0], (oh, ow)) / np.float32(255))[:, y0:y0 + ch, x0:x0 + cw])
        want_m = [resize_nearest(m, (oh, ow))[y0:y0 + ch, x0:x0 + cw] for m in src[3]]
        kept = [g for g in range(G) if want_m[g].any()]
        dropped += G - len(kept)
        np.testing.assert_array_equal(got[3], np.stack([want_m[g] for g in kept]) if kept else np.zeros((0, ch, cw), np.uint8))
        np.testing.assert_array_equal(got[1], np.array([_np_tight(want_m[g]) for g in kept], np.float32).reshape(-1, 4))
        np.testing.assert_array_equal(got[2], ex[2][kept])
        assert got[1].dtype == np.float32 and got[2].dtype == np.int32 and got[3].dtype == np.uint8 and got[4] == oh / H
        raw = RawTransform(_Sizes())(ex, AugmentParams(flip, None, None, (S, s, u_y, u_x)))     # the device path's host half
        assert raw[1] is None and raw[4:] == (oh / H, (ch, cw), int(flip), (oh, ow, y0, x0, ch, cw))
        np.testing.assert_array_equal(raw[0], img.transpose(1, 2, 0).astype(np.uint8))
        np.testing.assert_array_equal(raw[2], ex[2])
        np.testing.assert_array_equal(raw[3], np.stack(masks))
    assert dropped > 0


def test_cut_instances_end_at_the_window_and_vanished_ones_leave():
    H = W = 64
    img = np.zeros((3, H, W), np.float32)
    masks = [np.zeros((H, W), np.uint8) for _ in range(3)]
    masks[0][20:30, 22:28] = 1                               # x2: rows 40..59, columns 44..55 - inside the window below
    masks[1][4:12, 10:20] = 1                                # x2: rows 8..23, columns 20..39 - outside
    masks[2][28:60, 30:50] = 1                               # x2: rows 56..119, columns 60..99 - cut at the bottom right
    ex = (img, np.zeros((3, 4), np.float32), np.array([7, 8, 9], np.int32), masks)
    assert lsj_geometry(H, W, 64, 2.0, 0.5, 0.5) == (128, 128, 32, 32, 64, 64)
    got = Transform(_Sizes())(ex, AugmentParams(False, None, None, (64, 2.0, 0.5, 0.5)))
    np.testing.assert_array_equal(got[2], [7, 9])
    np.testing.assert_array_equal(got[1], [[8, 12, 28, 24], [24, 28, 64, 64]])
    assert got[3].shape == (2, 64, 64) and got[3][1, 63, 63] == 1 and got[3][1, 23, 63] == 0
    batch = collate([got], max_gt=3, canvas=64)              # an image may lose every instance: the batch row stays, empty
    np.testing.assert_array_equal(batch['labels'], [[7, 9, -1]])
    none = Transform(_Sizes())((img, ex[1][:1], ex[2][:1], masks[1:2]), AugmentParams(False, None, None, (64, 2.0, 0.5, 0.5)))
    assert none[1].shape == (0, 4) and none[2].shape == (0,) and none[3].shape == (0, 64, 64)
    small = Transform(_Sizes())(ex, AugmentParams(False, None, None, (128, 0.5, 0.5, 0.5)))     # smaller than the canvas: collate pads
    assert small[0].shape == (3, 64, 64)
    batch = collate([small], canvas=128)
    assert batch['imgs'].shape == (1, 3, 128, 128) and batch['masks'].shape == (1, 3, 128, 128) and tuple(batch['sizes'][0]) == (64, 64)
    assert not batch['imgs'][0, :, 64:].any() and not batch['masks'][0, :, :, 64:].any()


# ---- keypoint rule ------------------------------------------------------------------------------------------------------------------
def test_keypoint_rule_clips_boxes_drops_instances_and_hides_keypoints():
    H = W = 64
    img = np.zeros((3, H, W), np.float32)
    bbox = np.array([[10, 10, 40, 40],                       # x2: (20,20,80,80) -> window (32..96): (0,0,48,48): clipped at the top left
                     [2, 2, 12, 12],                         # x2: (4,4,24,24): left of the window: dropped
                     [20, 20, 30, 30]], np.float32)          # x2: (40,40,60,60) -> (8,8,28,28): inside
    kp = np.zeros((3, 17, 3), np.float32)
    kp[0, 0] = (30, 30, 2)                                   # (x,y) x2 = 60 -> 28: inside
    kp[0, 1] = (12, 30, 2)                                   # x x2 = 24 -> -8: leaves the window
    kp[0, 2] = (12, 30, 0)                                   # not labelled: stays as it is
    kp[2, 5] = (25, 22, 1)
    ex = (img, bbox, kp)
    p = AugmentParams(False, None, None, (64, 2.0, 0.5, 0.5))
    got = KeypointTransform(_Sizes())(ex, p)
    np.testing.assert_array_equal(got[1], [[0, 0, 48, 48], [8, 8, 28, 28]])
    assert got[3].shape == (2, 17, 3) and got[2].tolist() == [0, 0] and got[4] == 2.0 and got[0].shape == (3, 64, 64)
    np.testing.assert_array_equal(got[3][0, 0], (28, 28, 2))             # (y, x, v)
    np.testing.assert_array_equal(got[3][0, 1], (28, -8, 0))             # v = 0, the shifted coordinates stay
    np.testing.assert_array_equal(got[3][0, 2], (28, -8, 0))
    np.testing.assert_array_equal(got[3][1, 5], (12, 18, 1))
    raw = RawTransform(_Sizes(), keypoints=True)(ex, p)
    for k in (1, 2, 3):
        np.testing.assert_array_equal(raw[k], got[k])
    assert raw[4:] == (2.0, (64, 64), 0, (128, 128, 32, 32, 64, 64))
    # flipped, against the rule spelled out: flip and resize as ever, then shift, clip and drop
    perm = augment.flip_permutation(augment.COCO_KEYPOINT_NAMES)
    rs = np.random.RandomState(3)
    bbox = np.array([[5, 3, 30, 41], [0, 40, 37, 51], [30, 0, 36, 8]], np.float32)
    v = rs.randint(0, 3, (3, 17))
    kp = np.stack([rs.randint(0, 51, (3, 17)) * (v > 0), rs.randint(0, 37, (3, 17)) * (v > 0), v], 2)
    ex = (rs.randint(0, 256, (3, 37, 51)).astype(np.float32), bbox, kp)
    p = AugmentParams(True, None, perm, (64, 1.7, 0.8, 0.4))
    got = KeypointTransform(_Sizes())(ex, p)
    oh, ow, y0, x0, ch, cw = lsj_geometry(37, 51, 64, 1.7, 0.8, 0.4)
    fimg, fbox, fkp = hflip(ex, perm)
    b = resize_bbox(fbox, (37, 51), (oh, ow)) - np.array([y0, x0, y0, x0], np.float32)
    b[:, 0::2], b[:, 1::2] = np.clip(b[:, 0::2], 0, ch), np.clip(b[:, 1::2], 0, cw)
    keep = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
    assert 0 < keep.sum() < 3
    np.testing.assert_array_equal(got[1], b[keep])
    k = np.concatenate([fkp.astype(np.float32)[:, :, [1, 0]] * (oh / 37), fkp.astype(np.float32)[:, :, 2, None]], 2)
    k[:, :, 0] -= y0
    k[:, :, 1] -= x0
    out = (k[:, :, 0] < 0) | (k[:, :, 0] >= ch) | (k[:, :, 1] < 0) | (k[:, :, 1] >= cw)
    assert (out & (k[:, :, 2] > 0))[keep].any()
    k[:, :, 2][out] = 0
    np.testing.assert_array_equal(got[3], k[keep])
    np.testing.assert_array_equal(got[0], (resize_linear(fimg, (oh, ow)) / np.float32(255))[:, y0:y0 + ch, x0:x0 + cw])


# ---- host loader --------------------------------------------------------------------------------------------------------------------
def test_host_loader_with_lsj_collates_the_canvas_and_keeps_emptied_images(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader
    root = write_coco(str(tmp_path), n_img=5)
    ds = COCOMaskLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    aug = Augment(hflip_prob=0.5, seed=5, lsj_size=64, lsj_scale=(0.3, 3.0))
    tf = Transform(_Sizes())
    ld = BatchLoader(ds, tf, batch_size=2, shuffle=True, seed=2, num_workers=2, max_gt=4, augment=aug)
    try:
        batches = [next(ld) for _ in range(5)]
    finally:
        ld.close()
    order = np.concatenate([np.random.RandomState(2 + e).permutation(len(ds)) for e in range(2)])
    for b, batch in enumerate(batches):
        exs = [tf(ds[int(order[2 * b + j])], aug.params(0, 2 * b + j)) for j in range(2)]
        want = collate(exs, 4, canvas=64)
        assert want['imgs'].shape == (2, 3, 64, 64) and want['masks'].shape == (2, 4, 64, 64)
        for k in want:
            np.testing.assert_array_equal(batch[k], want[k], err_msg=k)
    # skip_empty is judged before augmentation: an image that loses its one instance to the crop stays, with every label -1; an image
    # without annotations is skipped as ever
    img = np.zeros((3, 64, 64), np.float32)
    corner = np.zeros((64, 64), np.uint8)
    corner[:2, :2] = 1
    data = [(img, np.array([[0, 0, 2, 2]], np.float32), np.array([4], np.int32), [corner]),
            (img, np.zeros((0, 4), np.float32), np.zeros((0,), np.int32), [])]
    aug = Augment(seed=1, lsj_size=64, lsj_scale=(2.0, 2.0))
    assert all(tf(data[0], aug.params(0, t))[1].shape[0] == 0 for t in (0, 2, 4))
    ld = BatchLoader(data, tf, batch_size=1, shuffle=False, num_workers=1, augment=aug)
    try:
        for _ in range(3):
            b = next(ld)
            assert b['labels'].tolist() == [[-1]] and not b['masks'].any() and not b['bboxes'].any()
        assert ld.ticket == 5                                # tickets 0, 2, 4 were served and 1, 3 skipped
    finally:
        ld.close()


# ---- train.py -----------------------------------------------------------------------------------------------------------------------
def _train_args(extra, keypoints=False):
    import train
    return train.build_parser(keypoints=keypoints).parse_args(['--label_file', '/nonexistent'] + extra)


def test_train_refuses_bad_lsj_flags_before_any_data_is_loaded():
    import train
    a = _train_args([])
    assert a.lsj_size == 0 and a.lsj_scale == [0.1, 2.0]
    on = ['--synthetic', '0', '--anno-dir', '/nonexistent', '--img-dir', '/nonexistent']
    for extra, word in ((['--lsj-size', '100'], 'multiple of 64'), (['--lsj-size', '-64'], 'multiple of 64'),
                        (['--lsj-size', '64', '--lsj-scale', '0', '2'], 'LO must be positive'),
                        (['--lsj-size', '64', '--lsj-scale', '-0.5', '2'], 'LO must be positive'),
                        (['--lsj-size', '64', '--lsj-scale', '1.5', '1.0'], 'LO must not exceed HI'),
                        (['--lsj-size', '64', '--min-sizes', '600', '800'], 'two different resize rules')):
        with pytest.raises(ValueError, match=word):
            train.run(_train_args(on + extra))
    with pytest.raises(ValueError, match='synthetic'):
        train.run(_train_args(['--lsj-size', '64']))
    with pytest.raises(ValueError, match='synthetic'):
        train.run(_train_args(['--lsj_size', '64'], keypoints=True), keypoints=True)
    with pytest.raises(ValueError, match='depth'):
        train.run(_train_args(on + ['--lsj-size', '64', '--dataset', 'depth'], keypoints=True), keypoints=True)
    assert _train_args(['--lsj_size', '128', '--lsj_scale', '0.5', '1.5'], keypoints=True).lsj_scale == [0.5, 1.5]
    train._check_augment_args(_train_args(['--synthetic', '0', '--lsj-size', '128', '--hflip', '1']))     # hflip combines freely


def test_augment_settings_record_lsj_only_when_it_is_on(tmp_path):
    import train
    assert train.augment_settings(_train_args([])) == train.NO_AUGMENT == {'hflip': 0, 'min_sizes': None, 'seed': train.AUGMENT_SEED}
    assert train.augment_settings(_train_args(['--hflip', '1', '--min-sizes', '600'])) == {'hflip': 1, 'min_sizes': [600],
                                                                                          'seed': train.AUGMENT_SEED}
    assert train.augment_settings(_train_args(['--lsj-scale', '0.5', '1.5'])) == train.NO_AUGMENT       # a range without a size: off
    on = train.augment_settings(_train_args(['--hflip', '1', '--lsj-size', '128', '--lsj-scale', '0.5', '1.5']))
    assert on == {'hflip': 1, 'min_sizes': None, 'seed': train.AUGMENT_SEED, 'lsj': {'size': 128, 'scale': [0.5, 1.5]}}
    ck = str(tmp_path / 'trainer_2.pt')
    torch.save({'iteration': 2, 'optimizer': {}, 'loader_ticket': [2], 'augment': on}, ck)
    for extra in (['--hflip', '1'], ['--hflip', '1', '--lsj-size', '128'], ['--hflip', '1', '--lsj-size', '64', '--lsj-scale', '0.5', '1.5'],
                  ['--hflip', '1', '--lsj-size', '128', '--lsj-scale', '0.5', '2']):
        with pytest.raises(ValueError, match='augmentation'):
            train.run(_train_args(['--synthetic', '0', '--resume', ck] + extra))


# ---- the crop entry points' argument checks -----------------------------------------------------------------------------------------
A16 = ctypes.c_void_p(4096)         # a non-null, 16-byte aligned address: never dereferenced, every call below fails before a launch
GOOD = (0, 4, 6, 16, 12, 0, 1, 3, 2, 8, 8)                   # (offset, H, W, oh, ow, flip, count, y0, x0, ch, cw) on an 8 x 8 canvas


def _image(row=GOOD, N=1, dst=(8, 8), out=A16, src=A16, src_bytes=10 ** 6, desc=True):
    d = ops.crop_descs([row[:6] + (0,) + row[7:]])           # (images carry no count)
    return _hip.lib().mrcnn_image_resize_crop_batch_u8_f32(src, src_bytes, d.ctypes.data if desc else None, N, out, dst[0], dst[1], 255.0, None)


def _boxes(row=GOOD, N=1, dst=(8, 8), G=2, Gin=2, labels_in=A16, bboxes=A16, labels=A16, gather=A16, ws=A16, src=A16, src_bytes=10 ** 6,
           desc=True):
    d = ops.crop_descs([row])
    return _hip.lib().mrcnn_mask_crop_boxes_u8(src, src_bytes, d.ctypes.data if desc else None, N, Gin, G, dst[0], dst[1], labels_in, bboxes,
                                               labels, gather, ws, None)


def _masks(row=GOOD, N=1, dst=(8, 8), G=2, gather=A16, out=A16, src=A16, src_bytes=10 ** 6, desc=True):
    d = ops.crop_descs([row])
    return _hip.lib().mrcnn_mask_resize_crop_batch_nearest_u8(src, src_bytes, d.ctypes.data if desc else None, N, G, gather, out, dst[0],
                                                              dst[1], None)


def test_crop_entry_points_refuse_bad_arguments_without_a_device():
    """Every call here carries exactly one bad argument and must come back MRCNN_E_INVALID from the host-side checks: none may reach a
    launch (the pointers are not memory)."""
    lib = _hip.lib()
    good = GOOD
    rows = {'ch > dst_h': good[:9] + (9, 8), 'cw > dst_w': good[:9] + (8, 9), 'y0 + ch > oh': good[:7] + (9, 2, 8, 8),
            'x0 + cw > ow': good[:7] + (3, 5, 8, 8), 'y0 < 0': good[:7] + (-1, 2, 8, 8), 'x0 < 0': good[:7] + (3, -1, 8, 8),
            'ch = 0': good[:9] + (0, 8), 'cw < 0': good[:10] + (-1,), 'H = 0': (0, 0) + good[2:], 'W < 0': good[:2] + (-6,) + good[3:],
            'oh = 0': good[:3] + (0,) + good[4:], 'ow = 0': good[:4] + (0,) + good[5:], 'flip = 2': good[:5] + (2,) + good[6:],
            'offset < 0': (-1,) + good[1:]}
    for call in (_image, _boxes, _masks):
        for name, row in rows.items():
            assert call(row) == -1, (call.__name__, name)
            assert lib.mrcnn_last_error()
        for kw in (dict(N=0), dict(N=33), dict(dst=(0, 8)), dict(dst=(8, -1)), dict(src=None), dict(src_bytes=23), dict(desc=False),
                   dict(row=(10 ** 6 - 23,) + good[1:])):      # (a 4 x 6 mask reads 24 bytes, the image 72)
            assert call(**kw) == -1, (call.__name__, kw)
    assert _image(out=None) == -1 and _image(out=ctypes.c_void_p(4100)) == -1
    assert _masks(out=None) == -1 and _masks(out=ctypes.c_void_p(4100)) == -1
    assert _masks(gather=None) == -1 and b'gather' in lib.mrcnn_last_error()
    assert _masks(G=0) == -1 and _masks(G=65536) == -1 and _masks(row=good[:6] + (-1,) + good[7:]) == -1
    for kw in (dict(labels_in=None), dict(bboxes=None), dict(labels=None), dict(gather=None), dict(ws=None), dict(ws=ctypes.c_void_p(4100)),
               dict(bboxes=ctypes.c_void_p(4100)), dict(G=0), dict(Gin=0), dict(Gin=65536), dict(row=good[:6] + (3,) + good[7:])):
        assert _boxes(**kw) == -1, kw                                       # (the last: count 3 > Gin 2)
    with pytest.raises(_hip.MrcnnHipError):                                 # no CPU fallback
        ops.image_resize_crop_batch_u8(torch.zeros(72, dtype=torch.uint8), ops.crop_descs([good]), 8, 8)
    assert ops.CROP_DESC.itemsize == 48 and ops.CROP_DESC.names[:7] == ops.RESIZE_DESC.names
    for name, n in (('mrcnn_image_resize_crop_batch_u8_f32', 9), ('mrcnn_mask_crop_boxes_u8', 14), ('mrcnn_mask_resize_crop_batch_nearest_u8', 10)):
        assert len(_hip.SIGNATURES[name][1]) == n


def test_crop_argument_checks_under_host_sanitizers(tmp_path):
    """The same checks, swept wider, in a stand-alone program (tests/native/lsj_host_check.cpp, its own main) built together with
    augment.hip and lib.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code (the device code is compiled as usual)
    and run on the CPU: every call is refused before a launch, so no device is touched."""
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    csrc = os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc')
    exe = str(tmp_path / 'lsj_host_check')
    subprocess.check_call([hipcc, '-std=c++17', '-O1', '-g', '--offload-arch=gfx950', '-ffp-contract=off', '-Xarch_host',
                           '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined', '-I' + os.path.join(ROOT, 'include'),
                           '-I' + csrc, os.path.join(csrc, 'augment.hip'), os.path.join(csrc, 'lib.hip'), '-x', 'c++',
                           os.path.join(ROOT, 'tests', 'native', 'lsj_host_check.cpp'), '-o', exe], cwd=str(tmp_path))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and b'lsj_host_check: ok' in r.stdout, r.stdout.decode('utf-8', 'replace')[-2000:]
