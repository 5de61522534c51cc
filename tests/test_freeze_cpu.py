"""Frozen-BatchNorm fine-tuning, the parts that need no device: the three entry points of csrc/bn_frozen.hip are exported and check
their arguments before any launch, ParamStore's frozen-block mask covers exactly the frozen parameters' 64-float blocks, and
train.py's --freeze-bn / --freeze-at handling (defaults, refused combinations, the 'freeze' key of the trainer state)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn import _hip  # noqa: E402

ENTRY_POINTS = ('mrcnn_bn_frozen_bwd_f32', 'mrcnn_bn_infer_fwd_pair_f32', 'mrcnn_bn_frozen_bwd_pair_f32', 'mrcnn_sgd_momentum_wd_masked_f32')


def test_entry_points_are_declared_and_exported():
    lib = _hip.lib()
    for name in ENTRY_POINTS:
        assert name in _hip.SIGNATURES, name
        assert getattr(lib, name) is not None


def _err(rc, code, word):
    msg = _hip.lib().mrcnn_last_error()
    assert rc == code, (rc, msg)
    assert word in msg, msg


def test_entry_points_check_their_arguments_without_a_device():
    lib = _hip.lib()
    buf = (ctypes.c_float * 1024)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16         # a 16-byte aligned host address: never dereferenced, the checks come first
    P, C, eps = 8, 8, 2e-5
    # ---- mrcnn_bn_frozen_bwd_f32(gy, yx, gamma, beta, avg_mean, avg_var, gx, gres, P, C, eps, relu, stream)
    _err(lib.mrcnn_bn_frozen_bwd_f32(None, a, a, a, a, a, a, None, P, C, eps, 1, None), -1, b'null')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a, None, a, a, a, a, a, None, P, C, eps, 1, None), -1, b'need the y / x')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a, a, a, None, None, a, a, None, P, C, eps, 2, None), -1, b'beta')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a, a, a, a, a, a, a, None, P, 6, eps, 1, None), -1, b'C%4')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a, a, a, a, a, a, a, None, 0, C, eps, 1, None), -1, b'P>0')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a, a, a, a, a, a, a, None, P, C, eps, 3, None), -1, b'relu')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a + 4, a, a, a, a, a, a, None, P, C, eps, 1, None), -1, b'aligned')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a, a, a, a, a, a, a + 8, None, P, C, eps, 1, None), -1, b'aligned')
    _err(lib.mrcnn_bn_frozen_bwd_f32(a, a, a, a, a, a, a, a, P, C, eps, 1, None), -1, b'gres')
    # ---- mrcnn_bn_infer_fwd_pair_f32(xa, ga, ba, ma, va, xb, gb, bb, mb, vb, y, P, C, eps, stream)
    y = a + 2048
    _err(lib.mrcnn_bn_infer_fwd_pair_f32(a, a, a, a, a, None, a, a, a, a, y, P, C, eps, None), -1, b'null')
    _err(lib.mrcnn_bn_infer_fwd_pair_f32(a, a, a, a, a, a, a, a, a, a, None, P, C, eps, None), -1, b'null')
    _err(lib.mrcnn_bn_infer_fwd_pair_f32(a, a, a, a, a, a, a, a, a, a, y, P, 10, eps, None), -1, b'C%4')
    _err(lib.mrcnn_bn_infer_fwd_pair_f32(a, a, a, a, a, a + 4, a, a, a, a, y, P, C, eps, None), -1, b'aligned')
    _err(lib.mrcnn_bn_infer_fwd_pair_f32(a, a, a, a, a, a, a, a, a, a, a, P, C, eps, None), -1, b'of its own')
    # ---- mrcnn_bn_frozen_bwd_pair_f32(gy, y, ga, va, gb, vb, gxa, gxb, P, C, eps, stream)
    _err(lib.mrcnn_bn_frozen_bwd_pair_f32(a, None, a, a, a, a, a, None, P, C, eps, None), -1, b'null')
    _err(lib.mrcnn_bn_frozen_bwd_pair_f32(a, None, a, a, a, a, a, y, P, 2, eps, None), -1, b'C%4')
    _err(lib.mrcnn_bn_frozen_bwd_pair_f32(a, a + 12, a, a, a, a, a, y, P, C, eps, None), -1, b'aligned')
    _err(lib.mrcnn_bn_frozen_bwd_pair_f32(a, None, a, a, a, a, y, y, P, C, eps, None), -1, b'different')
    # ---- mrcnn_sgd_momentum_wd_masked_f32(p, g, v, n, offset, frozen_blocks, n_blocks, lr, momentum, wd, stream)
    assert lib.mrcnn_sgd_momentum_wd_masked_f32(None, None, None, 0, 0, None, 0, 0.1, 0.9, 0.0, None) == 0      # n == 0: a no-op
    _err(lib.mrcnn_sgd_momentum_wd_masked_f32(a, a, None, 64, 0, a, 1, 0.1, 0.9, 0.0, None), -1, b'null')
    _err(lib.mrcnn_sgd_momentum_wd_masked_f32(a, a, a, 64, 0, None, 1, 0.1, 0.9, 0.0, None), -1, b'null')
    _err(lib.mrcnn_sgd_momentum_wd_masked_f32(a, a, a, 65, 0, a, 1, 0.1, 0.9, 0.0, None), -1, b'mask covers')
    _err(lib.mrcnn_sgd_momentum_wd_masked_f32(a, a, a, 64, 64, a, 1, 0.1, 0.9, 0.0, None), -1, b'mask covers')
    _err(lib.mrcnn_sgd_momentum_wd_masked_f32(a + 4, a, a, 64, 0, a, 1, 0.1, 0.9, 0.0, None), -1, b'aligned')
    _err(lib.mrcnn_sgd_momentum_wd_masked_f32(a, a, a, 60, 2, a, 1, 0.1, 0.9, 0.0, None), -1, b'aligned')     # element 2 sits 8 bytes past a boundary
    with pytest.raises(_hip.MrcnnHipError):
        _hip.check(-1)


def _store():
    from chainer_maskrcnn.nn.core import ParamStore
    ps = ParamStore()
    zeros = lambda shape: (lambda rs: np.zeros(shape, np.float32))
    shapes = [('a/W', (3, 50)), ('a/gamma', (32,)), ('a/beta', (32,)), ('b/W', (64,)), ('b/gamma', (65,)), ('c/W', (7, 7, 3)), ('c/b', (1,))]
    for name, shape in shapes:
        ps.register(name, shape, zeros(shape))
    ps.register('a/avg_mean', (32,), zeros((32,)), trainable=False)
    return ps.materialise('cpu'), shapes


def _bits(mask, n):
    words = mask.numpy().view(np.uint32)
    return np.array([(int(words[b // 32]) >> (b % 32)) & 1 for b in range(n)], bool)


def test_frozen_block_mask_covers_exactly_the_named_parameters():
    ps, shapes = _store()
    nblk = ps.size // ps.ALIGN
    assert ps.size % ps.ALIGN == 0 and nblk == 3 + 1 + 1 + 1 + 2 + 3 + 1
    assert ps.frozen_mask is None and ps.frozen == frozenset()
    frozen = ['a/gamma', 'b/gamma', 'c/b']
    mask = ps.frozen_block_mask(frozen)
    assert mask.dtype.is_floating_point is False and mask.numel() * 32 >= nblk
    got = _bits(mask, mask.numel() * 32)
    want = np.zeros_like(got)
    for name, shape in shapes:
        o = ps.offsets[name][0]
        n = int(np.prod(shape))
        assert o % ps.ALIGN == 0
        if name in frozen:
            want[o // 64:(o + n + 63) // 64] = True         # whole blocks, the padding behind the last element included
    assert np.array_equal(got, want)
    assert got.sum() == 1 + 2 + 1 and not got[nblk:].any()
    # b/gamma has 65 elements: two blocks; its neighbours b/W and c/W stay trainable
    ob = ps.offsets['b/gamma'][0] // 64
    assert got[ob] and got[ob + 1] and not got[ob - 1] and not got[ob + 2]
    assert not _bits(ps.frozen_block_mask([]), mask.numel() * 32).any()
    assert _bits(ps.frozen_block_mask([n for n, _ in shapes]), nblk).all()
    ps.set_frozen(frozen)
    assert ps.frozen == frozenset(frozen) and np.array_equal(ps.frozen_mask.numpy(), mask.numpy())
    ps.set_frozen(())
    assert ps.frozen_mask is None and ps.frozen == frozenset()
    with pytest.raises(KeyError):
        ps.set_frozen(['a/avg_mean'])           # a buffer, not a parameter of the flat store


@pytest.mark.parametrize('keypoints', [False, True], ids=['train.py', 'train_keypoints.py'])
def test_freeze_flags(keypoints):
    import train
    p = train.build_parser(keypoints=keypoints)
    a = p.parse_args([])
    assert a.freeze_bn == 0 and a.freeze_at == 0
    assert train.freeze_settings(a) == train.NO_FREEZE == {'bn': 0, 'at': 0}
    a = p.parse_args(['--freeze-bn', '1', '--freeze-at', '2'])
    assert train.freeze_settings(a) == {'bn': 1, 'at': 2}
    assert train.freeze_settings(p.parse_args(['--freeze-bn', '1'])) == {'bn': 1, 'at': 0}
    with pytest.raises(ValueError, match='freeze-bn'):
        train.freeze_settings(p.parse_args(['--freeze-at', '2']))
    for bad in ('6', '-1'):
        with pytest.raises(SystemExit):
            p.parse_args(['--freeze-bn', '1', '--freeze-at', bad])
    with pytest.raises(SystemExit):
        p.parse_args(['--freeze-bn', '2'])
    for bad in (6, -1):
        with pytest.raises(ValueError, match='0..5'):
            train.freeze_settings(argparse.Namespace(freeze_bn=1, freeze_at=bad))


def test_freeze_key_of_the_trainer_state(tmp_path):
    import torch
    import train
    record = [c for c in train.RESUME_CHECKS if c[0] == 'freeze'][0]            # (key, the record of a state without it, its noun) as run() checks it

    def check(resume, args, path=''):
        train.check_resume(resume, record[0], record[1], train.freeze_settings(args), record[2], path)
    p = train.build_parser()
    frozen, plain = p.parse_args(['--freeze-bn', '1', '--freeze-at', '2']), p.parse_args([])
    path = str(tmp_path / 'trainer_1.pt')
    torch.save({'iteration': 1, 'freeze': train.freeze_settings(frozen)}, path)
    state = torch.load(path, map_location='cpu', weights_only=False)
    assert state['freeze'] == {'bn': 1, 'at': 2}
    check(state, frozen, path)                                    # round trip: the same settings resume
    with pytest.raises(ValueError, match='freezing'):
        check(state, plain, path)
    with pytest.raises(ValueError, match='freezing'):
        check(state, p.parse_args(['--freeze-bn', '1']), path)
    old = {'iteration': 1}                                              # a state written before the key existed: nothing was frozen
    check(old, plain)
    with pytest.raises(ValueError, match='freezing'):
        check(old, frozen)


def test_run_refuses_a_frozen_prefix_without_frozen_batchnorm(tmp_path):
    import train
    a = train.build_parser().parse_args(['--freeze-at', '2', '--out', str(tmp_path / 'o'), '--iteration', '1'])
    with pytest.raises(ValueError, match='freeze-bn'):
        train.run(a)
    assert not (tmp_path / 'o').exists()            # refused before anything is built or written


def test_model_freeze_argument_handling():
    """FeaturePyramidNetwork.set_freeze on a store that is never materialised on a device: the names it leaves constant."""
    from chainer_maskrcnn.model.extractor.feature_pyramid_network import FeaturePyramidNetwork
    fpn = FeaturePyramidNetwork(stages=(2, 1, 1, 1), width_div=2)
    with pytest.raises(ValueError):
        fpn.set_freeze(False, 2)
    with pytest.raises(ValueError):
        fpn.set_freeze(True, 6)
    assert fpn.set_freeze(False, 0) == set() and not fpn.bn1.frozen
    names = fpn.set_freeze(True, 0)
    norms = {n for n in fpn.ps.offsets if n.endswith('/gamma') or n.endswith('/beta')}
    assert names == norms and len(norms) == 2 * (1 + 5 * 3 + 4)      # stem, five blocks of three, four projection shortcuts
    assert fpn.bn1.frozen and all(b.trained and all(n.frozen for n in b.norms()) for blocks in fpn.stages for b in blocks)
    names = fpn.set_freeze(True, 2)
    prefix = {n for n in fpn.ps.offsets if n.startswith('extractor/resnet/conv1/') or n.startswith('extractor/resnet/bn1/')
              or n.startswith('extractor/resnet/res2/')}
    assert names == norms | prefix and 'extractor/resnet/res2/b1/conv2/W' in names and 'extractor/resnet/res3/a/conv1/W' not in names
    assert [b.trained for blocks in fpn.stages for b in blocks] == [False, False, True, True, True]
    names = fpn.set_freeze(True, 5)
    assert {n for n in fpn.ps.offsets if '/resnet/' in n} == names and 'extractor/toplayer/W' not in names
    assert fpn.set_freeze(True, 1) == norms | {'extractor/resnet/conv1/W', 'extractor/resnet/conv1/b'}
    assert fpn.set_freeze(False, 0) == set() and not any(n.frozen for blocks in fpn.stages for b in blocks for n in b.norms())
