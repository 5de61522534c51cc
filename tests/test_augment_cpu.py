"""CPU tests of the training augmentation (dataset/augment.py): the name-based flip map, the host flip of mask and
keypoint examples, the per-ticket decisions as the BatchLoader makes them, the augmented host transforms, and train.py's refusals."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

from chainer_maskrcnn.dataset import augment  # noqa: E402
from chainer_maskrcnn.dataset.augment import Augment, AugmentParams, hflip  # noqa: E402
from chainer_maskrcnn.dataset.loader import BatchLoader  # noqa: E402
from chainer_maskrcnn.dataset.transforms import KeypointTransform, RawTransform, Transform  # noqa: E402
from tests.augment_data import write_coco  # noqa: E402


class _Sizes(object):
    min_size, max_size = 64, 100


def _sizes(min_size, max_size=_Sizes.max_size):
    import types
    return types.SimpleNamespace(min_size=min_size, max_size=max_size)


# ---- flip map -----------------------------------------------------------------------------------------------------------------------
def test_coco_flip_permutation():
    perm = augment.flip_permutation(augment.COCO_KEYPOINT_NAMES)
    assert perm.tolist() == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]


def test_depth_flip_permutation_pairs_all_eight_joints():
    names = augment.DEPTH_KEYPOINT_NAMES
    assert len(names) == 20
    perm = augment.flip_permutation(names)
    assert (perm[perm] == np.arange(20)).all()
    moved = [names[k] for k in range(20) if perm[k] != k]
    assert len(moved) == 16
    for side in ('Shoulder', 'Elbow', 'Wrist', 'Hand', 'Hip', 'Knee', 'Ankle', 'Foot'):
        assert names[perm[names.index(side + 'Left')]] == side + 'Right'
    for centre in ('SpineBase', 'SpineMid', 'Neck', 'Head'):
        assert perm[names.index(centre)] == names.index(centre)


def test_incomplete_names_are_refused():
    names = list(augment.COCO_KEYPOINT_NAMES)
    names[names.index('right_wrist')] = 'wrist'
    with pytest.raises(ValueError, match='left_wrist'):
        augment.flip_permutation(names)
    with pytest.raises(ValueError, match='no left / right'):
        augment.flip_permutation(['k%d' % i for i in range(17)])
    with pytest.raises(ValueError):
        augment.flip_permutation(['HandLeft', 'HandRight', 'HandLeft'])


# ---- host flip ----------------------------------------------------------------------------------------------------------------------
def _mask_example(rs, H=37, W=51, G=3):
    img = rs.randint(0, 256, (3, H, W)).astype(np.float32)
    bbox = np.array([[2, 3, 20, 17], [0, 0, H, W], [5, 30, 9, 50]], np.float32)[:G]
    masks = [(rs.rand(H, W) > 0.5).astype(np.uint8) for _ in range(G)]
    return img, bbox, np.arange(G, dtype=np.int32), masks


def _keypoint_example(rs, H=37, W=51, G=2):
    img = rs.randint(0, 256, (3, H, W)).astype(np.float32)
    bbox = np.array([[2, 3, 20, 17], [0, 10, H, W]], np.float32)[:G]
    v = rs.randint(0, 3, (G, 17))
    kp = np.stack([rs.randint(0, W, (G, 17)) * (v > 0), rs.randint(0, H, (G, 17)) * (v > 0), v], 2)
    return img, bbox, kp


def test_hflip_twice_is_the_identity():
    rs = np.random.RandomState(0)
    ex = _mask_example(rs)
    back = hflip(hflip(ex))
    np.testing.assert_array_equal(back[0], ex[0])
    np.testing.assert_array_equal(back[1], ex[1])
    np.testing.assert_array_equal(back[2], ex[2])
    for a, b in zip(back[3], ex[3]):
        np.testing.assert_array_equal(a, b)
    perm = augment.flip_permutation(augment.COCO_KEYPOINT_NAMES)
    kex = _keypoint_example(rs)
    once = hflip(kex, perm)
    assert not np.array_equal(once[2], kex[2])
    back = hflip(once, perm)
    for a, b in zip(back, kex):
        np.testing.assert_array_equal(a, b)
    assert back[2].dtype == kex[2].dtype


def test_flipped_rectangle_mask_matches_flipped_box():
    H, W = 20, 33
    m = np.zeros((H, W), np.uint8)
    m[4:9, 6:15] = 1                                     # columns [6, 15): box x1 = 6, x2 = 15
    img = np.zeros((3, H, W), np.float32)
    img[0, 4, 6] = 7.0
    out = hflip((img, np.array([[4, 6, 9, 15]], np.float32), np.zeros(1, np.int32), [m]))
    cols = np.flatnonzero(out[3][0].any(0))
    np.testing.assert_array_equal(out[1], [[4, W - 15, 9, W - 6]])
    assert cols[0] == out[1][0, 1] and cols[-1] + 1 == out[1][0, 3]
    assert out[0][0, 4, W - 1 - 6] == 7.0 and out[0].sum() == 7.0


def test_keypoint_flip_moves_channels_and_keeps_invisible_rows():
    names = augment.COCO_KEYPOINT_NAMES
    perm = augment.flip_permutation(names)
    W = 40
    kp = np.zeros((1, 17, 3), np.float32)
    lw, rw, nose, le, re = (names.index(n) for n in ('left_wrist', 'right_wrist', 'nose', 'left_eye', 'right_eye'))
    kp[0, lw] = (11, 5, 2)
    kp[0, nose] = (3, 4, 0)                              # v == 0: unchanged
    kp[0, le] = (7, 8, 0)                                # v == 0: moves to right_eye, coordinates kept
    img = np.zeros((3, 10, W), np.float32)
    out = hflip((img, np.zeros((1, 4), np.float32), kp), perm)[2]
    np.testing.assert_array_equal(out[0, rw], (W - 1 - 11, 5, 2))
    np.testing.assert_array_equal(out[0, lw], (0, 0, 0))
    np.testing.assert_array_equal(out[0, nose], (3, 4, 0))
    np.testing.assert_array_equal(out[0, re], (7, 8, 0))
    with pytest.raises(ValueError):
        hflip((img, np.zeros((1, 4), np.float32), kp))   # never flip coordinates without swapping channels


# ---- decisions ----------------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """Transform that writes its (flip, min_size) into the box of a dummy example."""

    def __call__(self, ex, aug=None):
        return (np.zeros((3, 8, 8), np.float32), np.array([[aug.flip, aug.min_size, 0, 0]], np.float32), np.zeros(1, np.int32),
                np.zeros((1, 8, 8), np.uint8), 1.0)


def _decisions(aug, n, workers, start=0, rank=0, world=1):
    ld = BatchLoader(list(range(13)), _Recorder(), batch_size=1, shuffle=True, seed=3, rank=rank, world=world, num_workers=workers,
                     start_ticket=start, augment=aug)
    try:
        return [tuple(next(ld)['bboxes'][0, 0, :2].astype(int)) for _ in range(n)]
    finally:
        ld.close()


def test_decisions_follow_the_ticket():
    aug = Augment(hflip_prob=0.5, min_sizes=[64, 80, 96], seed=11)
    a, b = _decisions(aug, 30, 1), _decisions(aug, 30, 3)
    assert a == b
    want = [tuple(int(x) for x in augment.decide(11, 0, t, 0.5, [64, 80, 96])) for t in range(30)]
    assert a == want
    assert _decisions(aug, 10, 2, start=17) == a[17:27]
    np.random.seed(0)                                      # the global generator plays no part
    assert _decisions(aug, 5, 2) == a[:5]
    assert _decisions(aug, 30, 2, rank=1, world=2) != a       # ranks draw their own decisions


def test_decision_rates():
    d = [augment.decide(7, 0, t, 0.5, [500, 600, 700]) for t in range(200)]
    flips = sum(f for f, _ in d)
    assert 70 <= flips <= 130
    assert {s for _, s in d} == {500, 600, 700}
    assert not any(augment.decide(7, 0, t, 0.0)[0] for t in range(50))
    assert all(augment.decide(7, 0, t, 1.0) == (True, None) for t in range(50))
    assert augment.decide(7, 0, 3, 0.5, [10, 20]) == augment.decide(7, 0, 3, 0.5, [10, 20])
    with pytest.raises(ValueError):
        Augment(min_sizes=[600, 0])


# ---- augmented transforms ----------------------------------------------------------------------------------------------------------
def test_transform_with_params_equals_transform_of_flipped_example():
    rs = np.random.RandomState(1)
    ex = _mask_example(rs)
    tf = Transform(_Sizes())
    for flip, min_size in ((True, 48), (True, None), (False, 80)):
        got = tf(ex, AugmentParams(flip, min_size))
        want = Transform(_sizes(min_size or _Sizes.min_size))(hflip(ex) if flip else ex)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        assert got[0].shape[1:] == RawTransform(_Sizes()).out_size(37, 51, min_size)
        if min_size == 48:
            assert min(got[0].shape[1:]) == 48                  # (80: the long side is capped at max_size)
    base = tf(ex)
    for a, b in zip(tf(ex, AugmentParams(False, None)), base):
        np.testing.assert_array_equal(a, b)
    # the device path's host half: same boxes, scale and size, the flip flag as a 7th item
    raw = RawTransform(_Sizes())(ex, AugmentParams(True, 48))
    got = tf(ex, AugmentParams(True, 48))
    np.testing.assert_array_equal(raw[1], got[1])
    assert raw[4] == got[4] and raw[5] == got[0].shape[1:] and raw[6] == 1
    np.testing.assert_array_equal(raw[0], ex[0].transpose(1, 2, 0).astype(np.uint8))        # the image is mirrored on the device
    assert len(RawTransform(_Sizes())(ex)) == 6


def test_keypoint_transforms_with_params():
    rs = np.random.RandomState(2)
    ex = _keypoint_example(rs)
    perm = augment.flip_permutation(augment.COCO_KEYPOINT_NAMES)
    p = AugmentParams(True, 48, perm)
    got = KeypointTransform(_Sizes())(ex, p)
    want = KeypointTransform(_sizes(48))(hflip(ex, perm))
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    raw = RawTransform(_Sizes(), keypoints=True)(ex, p)
    np.testing.assert_array_equal(raw[1], got[1])
    np.testing.assert_array_equal(raw[3], got[3])
    with pytest.raises(ValueError):
        KeypointTransform(_Sizes())(ex, AugmentParams(True, None))


def test_host_loader_with_augmentation_equals_transform_of_decisions(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader
    from chainer_maskrcnn.dataset.loader import collate
    root = write_coco(str(tmp_path), n_img=4)
    ds = COCOMaskLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    aug = Augment(hflip_prob=0.5, min_sizes=[48, 72], seed=5)
    tf = Transform(_Sizes())
    ld = BatchLoader(ds, tf, batch_size=2, shuffle=True, seed=2, num_workers=2, max_gt=4, augment=aug)
    try:
        batches = [next(ld) for _ in range(4)]
    finally:
        ld.close()
    order = np.concatenate([np.random.RandomState(2 + e).permutation(len(ds)) for e in range(2)])
    for b, batch in enumerate(batches):
        exs = [tf(ds[int(order[2 * b + j])], aug.params(0, 2 * b + j)) for j in range(2)]
        want = collate(exs, 4)
        for k in want:
            np.testing.assert_array_equal(batch[k], want[k], err_msg=k)


# ---- train.py -----------------------------------------------------------------------------------------------------------------------
def _train_args(extra, keypoints=False):
    import train
    return train.build_parser(keypoints=keypoints).parse_args(['--label_file', '/nonexistent'] + extra)


def test_train_refuses_augmentation_of_synthetic_batches():
    import train
    assert _train_args([]).hflip == 0 and _train_args([]).min_sizes is None
    with pytest.raises(ValueError, match='synthetic'):
        train.run(_train_args(['--hflip', '1']))
    with pytest.raises(ValueError, match='synthetic'):
        train.run(_train_args(['--min-sizes', '600', '800']), keypoints=False)
    with pytest.raises(ValueError, match='synthetic'):
        train.run(_train_args(['--hflip', '1'], keypoints=True), keypoints=True)
    with pytest.raises(ValueError, match='positive'):
        train.run(_train_args(['--synthetic', '0', '--min-sizes', '600', '-5']))
    with pytest.raises(SystemExit):
        _train_args(['--hflip', '2'])


def test_train_refuses_keypoint_flip_without_a_flip_map(tmp_path):
    import train
    root = write_coco(str(tmp_path), n_img=2, keypoint_names=['k%d' % i for i in range(17)])
    args = _train_args(['--synthetic', '0', '--hflip', '1', '--anno-dir', root + '/annotations', '--img-dir', root], keypoints=True)
    with pytest.raises(ValueError, match='flip map'):
        train.run(args, keypoints=True)
    names = list(augment.COCO_KEYPOINT_NAMES)
    names[names.index('left_knee')] = 'knee'
    root2 = write_coco(str(tmp_path / 'b'), n_img=2, keypoint_names=names)
    args = _train_args(['--synthetic', '0', '--hflip', '1', '--anno-dir', root2 + '/annotations', '--img-dir', root2], keypoints=True)
    with pytest.raises(ValueError, match='flip map'):
        train.run(args, keypoints=True)


def test_train_refuses_a_resume_with_other_augmentation(tmp_path):
    import train
    ck = str(tmp_path / 'trainer_2.pt')
    old = str(tmp_path / 'trainer_old.pt')
    torch.save({'iteration': 2, 'optimizer': {}, 'loader_ticket': [2],
                'augment': {'hflip': 1, 'min_sizes': [600, 800], 'seed': train.AUGMENT_SEED}}, ck)
    torch.save({'iteration': 2, 'optimizer': {}, 'loader_ticket': [2]}, old)       # written before augmentation existed
    for extra in (['--hflip', '1'], ['--hflip', '1', '--min-sizes', '600'], ['--min-sizes', '600', '800'], ['--hflip', '0']):
        with pytest.raises(ValueError, match='augmentation'):
            train.run(_train_args(['--synthetic', '0', '--resume', ck] + extra))
    with pytest.raises(ValueError, match='augmentation'):
        train.run(_train_args(['--synthetic', '0', '--resume', old, '--hflip', '1']))
    assert train.augment_settings(_train_args([])) == train.NO_AUGMENT
