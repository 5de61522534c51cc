"""The optimizer-side recipe without a device: LRSchedule against a table written out by hand, the periodic x0.1 of --lr-shift-interval as
a schedule, the new command-line flags of both parsers and the combinations they refuse, the GradientClipping hook's argument check."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import train  # noqa: E402
from chainer_maskrcnn.optimizers import GradientClipping, LRSchedule, MomentumSGD, WeightDecay  # noqa: E402


def test_lr_schedule_against_a_hand_written_table():
    """W = 4, F = 0.25, steps (6, 8), base 0.02: w = 0.25 + 0.75 * (it - 1) / 4 in the warmup; the drop of step s acts from s + 1."""
    s = LRSchedule(0.02, warmup_iterations=4, warmup_factor=0.25, steps=(6, 8), gamma=0.1)
    table = {1: 0.02 * 0.25, 2: 0.02 * 0.4375, 3: 0.02 * 0.625, 4: 0.02 * 0.8125, 5: 0.02, 6: 0.02, 7: 0.002, 8: 0.002, 9: 0.0002, 10: 0.0002}
    for it, want in table.items():
        assert s.lr_at(it) == pytest.approx(want, rel=1e-12), it
    warm = [s.lr_at(it) for it in range(1, 6)]
    assert all(a < b for a, b in zip(warm, warm[1:]))          # monotone in the warmup ...
    assert s.lr_at(5) == 0.02 and s.lr_at(6) == 0.02            # ... and exactly base_lr from W + 1 until the first drop
    with pytest.raises(ValueError):
        s.lr_at(0)


def test_lr_schedule_defaults_are_constant():
    s = LRSchedule(0.01)
    assert [s.lr_at(it) for it in (1, 2, 1000)] == [0.01] * 3
    assert LRSchedule(0.01, warmup_iterations=3).lr_at(1) == pytest.approx(0.01 / 3, rel=1e-12)


@pytest.mark.parametrize('N', [1, 3, 7])
def test_lr_shift_interval_is_a_step_schedule(N):
    """train.py --lr-shift-interval N multiplies lr by 0.1 behind every N-th iteration; LRSchedule(steps = N, 2N, ...) gives the same learning
    rates (relative 1e-12: repeated `*= 0.1` and `gamma ** n` round differently in double)."""
    iters = 5 * N + 2
    s = LRSchedule(1e-3, steps=range(N, iters + 1, N))
    lr = 1e-3
    for it in range(1, iters + 1):
        assert s.lr_at(it) == pytest.approx(lr, rel=1e-12), it
        if it % N == 0:         # the loop of train.run
            lr *= 0.1


@pytest.mark.parametrize('keypoints', [False, True])
def test_parsers_accept_the_new_flags(keypoints):
    p = train.build_parser(keypoints)
    d = p.parse_args([])
    assert (d.accum_steps, d.grad_clip, d.warmup_iterations, d.lr_steps) == (1, 0.0, 0, None) and d.warmup_factor == pytest.approx(1 / 3)
    assert train.optim_settings(d) == (train.NO_OPTIM, None)
    a = p.parse_args('--accum-steps 4 --grad-clip 35 --warmup-iterations 500 --warmup-factor 0.001 --lr-steps 60000 80000 --lr 0.02'.split())
    assert (a.accum_steps, a.grad_clip, a.warmup_iterations, a.warmup_factor, a.lr_steps) == (4, 35.0, 500, 0.001, [60000, 80000])
    rec, sched = train.optim_settings(a)
    assert rec['accum_steps'] == 4 and rec['grad_clip'] == 35.0 and rec['schedule']['steps'] == [60000, 80000]
    assert sched.lr_at(501) == 0.02 and sched.lr_at(1) == pytest.approx(0.02 * 0.001) and sched.lr_at(80001) == pytest.approx(0.0002)
    if keypoints:               # train_keypoints.py's spelling
        b = p.parse_args('--accum_steps 4 --grad_clip 35 --warmup_iterations 500 --warmup_factor 0.001 --lr_steps 60000 80000 --lr 0.02'.split())
        assert train.optim_settings(b)[0] == rec


@pytest.mark.parametrize('keypoints', [False, True])
@pytest.mark.parametrize('flags', ['--lr-steps 5 --lr-shift-interval 3', '--accum-steps 0', '--grad-clip -1', '--warmup-iterations -2'])
def test_refused_combinations(keypoints, flags):
    with pytest.raises(ValueError):
        train.optim_settings(train.build_parser(keypoints).parse_args(flags.split()))


def test_warmup_in_front_of_lr_shift_interval_keeps_the_periodic_drops():
    a = train.build_parser().parse_args('--warmup-iterations 2 --warmup-factor 0.5 --lr-shift-interval 3 --iteration 7 --lr 0.1'.split())
    _, s = train.optim_settings(a)
    assert [s.lr_at(it) for it in range(1, 8)] == pytest.approx([0.05, 0.075, 0.1, 0.01, 0.01, 0.01, 0.001], rel=1e-12)


def test_resume_with_another_recipe_is_refused():
    record = [c for c in train.RESUME_CHECKS if c[0] == 'optim'][0]             # (key, the record of a state without it, its noun) as run() checks it

    def check(resume, args, path=''):
        train.check_resume(resume, record[0], record[1], train.optim_settings(args)[0], record[2], path)
    p = train.build_parser()
    a = p.parse_args('--accum-steps 2'.split())
    check({'optim': train.optim_settings(a)[0]}, a)
    check({}, p.parse_args([]))                               # a state from before the key existed: all off
    with pytest.raises(ValueError, match='optimizer recipe'):
        check({}, a)
    with pytest.raises(ValueError, match='optimizer recipe'):
        check({'optim': train.optim_settings(a)[0]}, p.parse_args('--accum-steps 2 --grad-clip 5'.split()))


def test_hooks():
    for bad in (0, 0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            GradientClipping(bad)
    opt = MomentumSGD()
    assert opt.clip_threshold == 0.0 and opt.pending == 0 and not opt.uses_hyper_block and opt.grad_norm is None
    opt.add_hook(GradientClipping(2.5))
    opt.add_hook(WeightDecay(5e-4))
    assert opt.clip_threshold == 2.5 and opt.weight_decay == 5e-4 and opt.uses_hyper_block
    assert MomentumSGD(device_lr=True).uses_hyper_block
    with pytest.raises(TypeError):
        opt.add_hook(object())


def test_kernel_entry_points_refuse_bad_arguments_without_a_device():
    """csrc/optim.hip checks its arguments before any launch (the addresses below are never dereferenced): null pointers, sections that
    are not element `offset` of a 16-byte aligned buffer, a mask that does not cover the section, a workspace that is too small."""
    import ctypes
    from chainer_maskrcnn import _hip
    lib, V, A = _hip.lib(), ctypes.c_void_p, 0x10000
    n, nb = 3200, 64
    ws = lib.mrcnn_grad_norm_workspace_bytes(n)
    assert ws == 8 * 4 and lib.mrcnn_grad_norm_workspace_bytes(1) == 8 and lib.mrcnn_grad_norm_workspace_bytes(1 << 30) == 8 * 4096
    bad = [lib.mrcnn_grad_accumulate_f32(None, V(A), n, 0, None, 0, 1, None),
           lib.mrcnn_grad_accumulate_f32(V(A), V(A), n, 0, None, 0, 0, None),
           lib.mrcnn_grad_accumulate_f32(V(A + 4), V(2 * A + 4), n - 1, 0, None, 0, 1, None),
           lib.mrcnn_grad_accumulate_f32(V(A), V(2 * A), n, 64 * 20, V(3 * A), nb, 1, None),
           lib.mrcnn_grad_norm_hyper_f32(None, None, n, 0, None, 0, V(A), V(2 * A), ws, None),
           lib.mrcnn_grad_norm_hyper_f32(None, V(A), n, 0, None, 0, None, V(2 * A), ws, None),
           lib.mrcnn_grad_norm_hyper_f32(None, V(A), n, 0, None, 0, V(3 * A), V(2 * A), ws - 1, None),
           lib.mrcnn_grad_norm_hyper_f32(None, V(A), n, 0, None, 0, V(3 * A), None, ws, None),
           lib.mrcnn_grad_norm_hyper_f32(None, V(A), 0, 0, None, 0, V(3 * A), V(2 * A), ws, None),
           lib.mrcnn_grad_norm_hyper_f32(V(4 * A + 8), V(A), n - 2, 0, None, 0, V(3 * A), V(2 * A), ws, None),
           lib.mrcnn_sgd_momentum_wd_hyper_f32(V(A), None, V(2 * A), V(3 * A), n, 0, None, 0, None, 0.9, 5e-4, None),
           lib.mrcnn_sgd_momentum_wd_hyper_f32(V(A), None, None, V(3 * A), n, 0, None, 0, V(4 * A), 0.9, 5e-4, None),
           lib.mrcnn_sgd_momentum_wd_hyper_f32(V(A + 4), None, V(2 * A + 4), V(3 * A + 4), n - 1, 2, None, 0, V(4 * A), 0.9, 5e-4, None),
           lib.mrcnn_sgd_momentum_wd_hyper_f32(V(A), None, V(2 * A), V(3 * A), n, 0, V(5 * A), nb // 2, V(4 * A), 0.9, 5e-4, None)]
    assert bad == [-1] * len(bad), bad
    assert b'mask' in lib.mrcnn_last_error()
    with pytest.raises(_hip.MrcnnHipError):
        _hip.check(bad[0])
    # n == 0 is a no-op of the two streaming entry points
    assert lib.mrcnn_grad_accumulate_f32(None, None, 0, 0, None, 0, 1, None) == 0
    assert lib.mrcnn_sgd_momentum_wd_hyper_f32(None, None, None, None, 0, 0, None, 0, None, 0.9, 5e-4, None) == 0
