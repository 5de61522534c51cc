"""Gradient accumulation, gradient-norm clipping and the device-resident learning rate on the device (csrc/optim.hip,
chainer_maskrcnn/optimizers.py): the kernels bit for bit against torch / the existing update kernels / a NumPy float32 restatement, the
norm against float64 NumPy to one float32 ulp, and the step: accumulate + update against the emulation that clones every gradient,
the hyper-block path against the ordinary step, clipping, the data-parallel bucket walk, graph replay with a changing learning rate, the
command line."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn import _hip  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss  # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay, GradientClipping, GraphedStep, LRSchedule  # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch  # noqa: E402

DEV = 'cuda:0'
F = np.float32
LR, MOM, WD = 1e-2, 0.9, 5e-4


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np_bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---- 1. kernels -------------------------------------------------------------------------------------------------------------------------
# the sections of tests/test_freeze_gpu.py::test_masked_sgd_kernel over a 50-block buffer (tails, an unaligned `offset`, sections shorter
# than a float4 group), and two sections of a buffer of 4.2 M floats: more float4 groups than the element-wise grid's 4096 x 256 threads
# (the grid-stride loop wraps) like the norm's
SMALL = [(0, 64 * 50), (128, 64 * 31), (100, 2996), (64 * 7 + 4, 64 * 44 + 60), (101, 2999), (3, 70), (130, 133)]
BIG_BLOCKS = 65600
BIG = [(0, 64 * BIG_BLOCKS), (37, 64 * BIG_BLOCKS - 5)]
CASES = [(50, s, e) for s, e in SMALL] + [(BIG_BLOCKS, s, e) for s, e in BIG]


def _case(nblk, seed, masked):
    """Flat buffers of nblk 64-float blocks, a frozen-block mask with runs (or None), and the per-element frozen flags."""
    n = 64 * nblk
    g_ = torch.Generator(device='cpu').manual_seed(seed)
    bufs = [torch.randn(n, generator=g_) for _ in range(4)]
    if not masked:
        return n, bufs, None, torch.zeros(n, dtype=torch.bool)
    frozen = torch.rand(nblk, generator=g_) < 0.4
    frozen[[0, 1, 2, 7, 46]] = torch.tensor([False, True, False, True, False])
    frozen[10:16] = True                                        # a run of frozen blocks
    bits = np.zeros((nblk + 31) // 32 * 32, bool)
    bits[:nblk] = frozen.numpy()
    mask = torch.from_numpy(np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view('<u4').reshape(-1).view(np.int32).copy()).to(DEV)
    return n, bufs, mask, frozen.repeat_interleave(64)


def _hyper(lr=LR, a=1.0, threshold=float('inf'), scale=1.0):
    h = torch.zeros(ops.HYPER_FLOATS, dtype=torch.float32)
    h[ops.HYPER_LR], h[ops.HYPER_A], h[ops.HYPER_THRESHOLD], h[ops.HYPER_SCALE] = lr, a, threshold, scale
    return h.to(DEV)


def _skipped(h):
    return int(h[ops.HYPER_SKIPPED:ops.HYPER_SKIPPED + 1].view(torch.int32).item())


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('nblk,start,end', CASES, ids=lambda v: str(v))
def test_accumulate_kernel(nblk, start, end, masked):
    """acc = g, then acc = acc + g: the bits of torch's float32 add; frozen blocks (their g is NaN) and everything outside the section keep
    what they held."""
    n, (a0, g0, g1, _), mask, elem_frozen = _case(nblk, 17, masked)
    inside = torch.zeros(n, dtype=torch.bool)
    inside[start:end] = True
    upd = inside & ~elem_frozen
    assert upd.any()
    for g in (g0, g1):
        g[elem_frozen] = float('nan')
    acc, d0, d1 = a0.to(DEV), g0.to(DEV), g1.to(DEV)
    ops.grad_accumulate(acc[start:end], d0[start:end], start, mask, first=True)
    got = acc.cpu()
    assert torch.equal(_bits(got)[upd], _bits(g0)[upd]) and torch.equal(_bits(got)[~upd], _bits(a0)[~upd])
    ops.grad_accumulate(acc[start:end], d1[start:end], start, mask, first=False)
    got = acc.cpu()
    assert torch.equal(_bits(got)[upd], _bits(g0 + g1)[upd]) and torch.equal(_bits(got)[~upd], _bits(a0)[~upd])
    assert _same_bits(d0, g0) and _same_bits(d1, g1)            # the gradient is only read


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('nblk,start,end', CASES, ids=lambda v: str(v))
def test_update_kernel_with_unit_scale_has_the_bits_of_the_existing_kernels(nblk, start, end, masked):
    n, (p0, g0, v0, _), mask, elem_frozen = _case(nblk, 23, masked)
    inside = torch.zeros(n, dtype=torch.bool)
    inside[start:end] = True
    upd = inside & ~elem_frozen
    pr, vr = p0.to(DEV), v0.to(DEV)
    if masked:
        ops.sgd_momentum_wd_masked(pr, g0.to(DEV), vr, 0, mask, LR, MOM, WD)
    else:
        ops.sgd_momentum_wd(pr, g0.to(DEV), vr, LR, MOM, WD)
    g_nan = g0.clone()
    g_nan[elem_frozen] = float('nan')
    p, g, v = p0.to(DEV), g_nan.to(DEV), v0.to(DEV)
    ops.sgd_momentum_wd_hyper(p[start:end], g[start:end], v[start:end], _hyper(scale=1.0), None, start, mask, MOM, WD)
    for got, ref, old in ((p, pr, p0), (v, vr, v0)):
        got, ref = got.cpu(), ref.cpu()
        assert torch.equal(_bits(got)[upd], _bits(ref)[upd])
        assert torch.equal(_bits(got)[~upd], _bits(old)[~upd])
        assert torch.isfinite(got).all()
    assert not torch.equal(_bits(p.cpu())[upd], _bits(p0)[upd])


def _np_update(p, acc, g, v, lr, scale, mom=MOM, wd=WD):
    """The three lines of the kernel in NumPy float32 (no fused multiply-add on either side)."""
    lr, scale, mom, wd = F(lr), F(scale), F(mom), F(wd)
    ge = acc + g if acc is not None else g
    gs = ge * scale
    v2 = mom * v - lr * (gs + wd * p)
    assert gs.dtype == np.float32 and v2.dtype == np.float32
    return p + v2, v2


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('nblk,start,end', CASES, ids=lambda v: str(v))
def test_update_kernel_with_accumulator_and_scale_is_the_restatement(nblk, start, end, masked):
    n, (p0, g0, v0, a0), mask, elem_frozen = _case(nblk, 29, masked)
    inside = torch.zeros(n, dtype=torch.bool)
    inside[start:end] = True
    upd = (inside & ~elem_frozen).numpy()
    lr, scale = 0.0123, 0.37
    want_p, want_v = _np_update(p0.numpy(), a0.numpy(), g0.numpy(), v0.numpy(), lr, scale)
    g_nan, a_nan = g0.clone(), a0.clone()
    g_nan[elem_frozen] = float('nan')
    a_nan[elem_frozen] = float('nan')
    p, g, v, acc = p0.to(DEV), g_nan.to(DEV), v0.to(DEV), a_nan.to(DEV)
    ops.sgd_momentum_wd_hyper(p[start:end], g[start:end], v[start:end], _hyper(lr=lr, scale=scale), acc[start:end], start, mask, MOM, WD)
    for got, want, old in ((p, want_p, p0), (v, want_v, v0)):
        got = got.cpu().numpy()
        assert _np_bits_equal(got[upd], want[upd]) and _np_bits_equal(got[~upd], old.numpy()[~upd])
    assert _same_bits(acc, a_nan) and _same_bits(g, g_nan)      # the accumulator and the gradient are only read


def _ulp_apart(a, b):
    a, b = F(a), F(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize('with_acc', [False, True], ids=['g', 'acc+g'])
@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('nblk,start,end', CASES, ids=lambda v: str(v))
def test_norm_kernel(nblk, start, end, masked, with_acc):
    """norm = (float)sqrt(sum in double) * a within ONE float32 ulp of float64 NumPy (derived, not measured: the double sum's relative
    error is ~1e-16 * n, far below half a float32 ulp, so only the final roundings can differ); rate and scale follow from the device's own
    norm by the two float32 expressions; the same bits on a second call; NaN in frozen blocks is not seen."""
    n, (_, g0, _, a0), mask, elem_frozen = _case(nblk, 31, masked)
    g_nan, a_nan = g0.clone(), a0.clone()
    g_nan[elem_frozen] = float('nan')
    a_nan[elem_frozen] = float('nan')
    g, acc = g_nan.to(DEV), (a_nan.to(DEV) if with_acc else None)
    live = ~elem_frozen[start:end].numpy()
    ge = (a0 + g0 if with_acc else g0).numpy()[start:end][live]             # float32 sum, like the kernel's
    norm64 = np.sqrt(np.sum(ge.astype(np.float64) ** 2))
    ws = ops.grad_norm_workspace(end - start, g.device)
    for a, thr in ((1.0, float('inf')), (0.25, float(norm64) * 0.25 * 0.5), (1.0, float(norm64) * 2)):
        hs = []
        for _ in range(2):
            h = _hyper(a=a, threshold=thr, scale=123.0)
            ops.grad_norm_hyper(g[start:end], h, None if acc is None else acc[start:end], start, mask, ws=ws)
            hs.append(h.cpu())
        assert _same_bits(hs[0], hs[1])
        h = hs[0].numpy()
        norm = h[ops.HYPER_NORM]
        want = F(norm64) * F(a)
        print('norm', norm, 'float64 reference', norm64 * a, 'ulps apart', _ulp_apart(norm, want))
        assert _ulp_apart(norm, want) <= 1
        rate = F(thr) / norm if norm > F(thr) else F(1.0)
        assert _np_bits_equal(h[ops.HYPER_RATE], F(rate)) and _np_bits_equal(h[ops.HYPER_SCALE], F(a) * F(rate))
        assert (rate < 1) == (thr < norm64 * a) and _skipped(hs[0]) == 0
        assert h[ops.HYPER_LR] == F(LR) and h[ops.HYPER_A] == F(a)            # what the host placed stays


@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')])
@pytest.mark.parametrize('where', [0, 3, 777, 64 * 50 - 1], ids=lambda v: 'at%d' % v)
def test_norm_kernel_skips_a_non_finite_gradient(bad, where):
    n, (p0, g0, v0, _), mask, _ = _case(50, 37, False)
    g0[where] = bad
    g, h = g0.to(DEV), _hyper(threshold=1.0, scale=5.0)
    ws = ops.grad_norm_workspace(n, g.device)
    ops.grad_norm_hyper(g[3:], h, None, 3, None, ws=ws) if where >= 3 else ops.grad_norm_hyper(g, h, None, 0, None, ws=ws)
    assert float(h[ops.HYPER_SCALE]) == 0.0 and float(h[ops.HYPER_RATE]) == 0.0 and _skipped(h) == 1
    ops.grad_norm_hyper(g, h, None, 0, None, ws=ws)
    assert _skipped(h) == 2 and not np.isfinite(float(h[ops.HYPER_NORM]))
    # the update that follows takes the gradient as zero: momentum decays, weight decay acts, nothing becomes non-finite
    p, v = p0.to(DEV), v0.to(DEV)
    ops.sgd_momentum_wd_hyper(p, g, v, h, None, 0, None, MOM, WD)
    want_p, want_v = _np_update(p0.numpy(), None, np.zeros(n, F), v0.numpy(), LR, 1.0)
    assert _np_bits_equal(p.cpu().numpy(), want_p) and _np_bits_equal(v.cpu().numpy(), want_v)


def test_kernel_argument_errors():
    n, (p0, g0, v0, a0), mask, _ = _case(50, 41, True)
    p, g, v, acc, h = p0.to(DEV), g0.to(DEV), v0.to(DEV), a0.to(DEV), _hyper()
    lib, ptr, sp = _hip.lib(), _hip.ptr, _hip.stream_ptr
    ws = ops.grad_norm_workspace(n, g.device)
    before = [t.clone() for t in (p, g, v, acc, h)]
    nb = mask.numel() * 32
    bad = [
        lib.mrcnn_grad_accumulate_f32(None, ptr(g), n, 0, None, 0, 1, sp()),
        lib.mrcnn_grad_accumulate_f32(ptr(acc), ptr(acc), n, 0, None, 0, 0, sp()),
        lib.mrcnn_grad_accumulate_f32(ptr(acc[1:]), ptr(g[1:]), n - 1, 0, None, 0, 1, sp()),              # not element 0 of an aligned buffer
        lib.mrcnn_grad_accumulate_f32(ptr(acc), ptr(g), n, 64 * 20, ptr(mask), nb, 1, sp()),              # runs past the mask
        lib.mrcnn_grad_norm_hyper_f32(None, None, n, 0, None, 0, ptr(h), ptr(ws), ws.numel(), sp()),
        lib.mrcnn_grad_norm_hyper_f32(None, ptr(g), n, 0, None, 0, None, ptr(ws), ws.numel(), sp()),
        lib.mrcnn_grad_norm_hyper_f32(None, ptr(g), n, 0, None, 0, ptr(h), ptr(ws), 0, sp()),             # workspace too small
        lib.mrcnn_grad_norm_hyper_f32(None, ptr(g), n, 0, None, 0, ptr(h), None, ws.numel(), sp()),
        lib.mrcnn_grad_norm_hyper_f32(None, ptr(g), 0, 0, None, 0, ptr(h), ptr(ws), ws.numel(), sp()),
        lib.mrcnn_grad_norm_hyper_f32(ptr(acc[2:]), ptr(g), n - 2, 0, None, 0, ptr(h), ptr(ws), ws.numel(), sp()),
        lib.mrcnn_sgd_momentum_wd_hyper_f32(ptr(p), None, ptr(g), ptr(v), n, 0, None, 0, None, MOM, WD, sp()),
        lib.mrcnn_sgd_momentum_wd_hyper_f32(ptr(p), None, None, ptr(v), n, 0, None, 0, ptr(h), MOM, WD, sp()),
        lib.mrcnn_sgd_momentum_wd_hyper_f32(ptr(p[1:]), None, ptr(g[1:]), ptr(v[1:]), n - 1, 2, None, 0, ptr(h), MOM, WD, sp()),
        lib.mrcnn_sgd_momentum_wd_hyper_f32(ptr(p), None, ptr(g), ptr(v), n, 0, ptr(mask), nb // 2, ptr(h), MOM, WD, sp()),
    ]
    assert bad == [-1] * len(bad), bad
    with pytest.raises(_hip.MrcnnHipError, match='mask'):
        _hip.check(bad[-1])
    assert lib.mrcnn_grad_norm_workspace_bytes(1) == 8 and lib.mrcnn_grad_norm_workspace_bytes(1 << 30) == 8 * 4096
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip((p, g, v, acc, h), before))


# ---- 2. the step ------------------------------------------------------------------------------------------------------------------------
SHRINK = dict(stages=(1, 1, 1, 1), width_div=2)


def _image(r):
    b = make_batch(40 + r, 1, 128, 160, G=3)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
    return [torch.from_numpy(b[k]).to(DEV) for k in ('imgs', 'bboxes', 'labels', 'masks')]


def _setup(freeze=False, **kw):
    model = MaskRCNN(n_fg_class=80, device=DEV, seed=7, _test_shrink=SHRINK)
    chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss)
    chain.proposal_target_creator.set_seed(100)
    chain.anchor_target_creator.set_seed(200)
    if freeze:
        model.freeze(True, 2)
    opt = MomentumSGD(lr=LR, momentum=MOM, **kw).setup(chain)
    opt.add_hook(WeightDecay(WD))
    return model, chain, opt


def _gradient(chain, batch):
    """One micro-batch's gradient the way MomentumSGD.update produces it (tests/dp/worker.py: run_emu), cloned."""
    chain.backward_follows = chain.unit_upstream = True
    try:
        chain(*batch, 1.0).backward()
    finally:
        chain.backward_follows = chain.unit_upstream = False
    torch.cuda.synchronize()
    return chain.faster_rcnn.ps.grads.clone()


def _trainable(model):
    m = model.ps.frozen_mask
    if m is None:
        return torch.ones(model.ps.params.numel(), dtype=torch.bool)
    words = m.cpu().numpy().view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder='little')
    return ~torch.from_numpy(np.repeat(bits.astype(bool), 64)[:model.ps.params.numel()].copy())


def _state(model):
    torch.cuda.synchronize()
    return model.ps.params.clone(), model.ps.momentum.clone()


def _assert_same_state(a, b):
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


@pytest.mark.parametrize('freeze', [False, True], ids=['all_trainable', 'freeze_bn_at_2'])
def test_accumulate_then_update_equals_the_cloned_gradient_emulation(freeze):
    batches = [_image(0), _image(1)]
    model, chain, opt = _setup(freeze)
    p0 = model.ps.params.clone()
    for _ in range(3):
        t = opt.t
        loss = opt.accumulate(chain, *batches[0], 1.0)
        assert opt.pending == 1 and opt.t == t and torch.is_tensor(loss)
        opt.update(chain, *batches[1], 1.0)
        assert opt.pending == 0 and opt.t == t + 1
    got = _state(model)
    model_e, chain_e, opt_e = _setup(freeze)
    assert _same_bits(model_e.ps.params, p0)
    live = _trainable(model_e).to(DEV)
    for _ in range(3):
        g0, g1 = _gradient(chain_e, batches[0]), _gradient(chain_e, batches[1])
        model_e.ps.grads.copy_(g0 + g1)
        opt_e.update()
    _assert_same_state(got, _state(model_e))
    assert not _same_bits(got[0], p0)
    if freeze:
        assert not live.all() and _same_bits(got[0][~live], p0[~live])


def test_accumulate_leaves_parameters_alone_and_update_without_lossfun_applies_the_accumulator():
    batches = [_image(0), _image(1)]
    model, chain, opt = _setup()
    before = _state(model)
    opt.accumulate(chain, *batches[0], 1.0)
    opt.accumulate(chain, *batches[1], 1.0)
    _assert_same_state(before, _state(model))
    assert opt.pending == 2
    with pytest.raises(RuntimeError, match='waiting'):
        opt.state_dict()
    opt.update()
    assert opt.pending == 0 and opt.t == 1
    model_e, chain_e, opt_e = _setup()
    g0, g1 = _gradient(chain_e, batches[0]), _gradient(chain_e, batches[1])
    model_e.ps.grads.copy_(g0 + g1)
    opt_e.update()
    _assert_same_state(_state(model), _state(model_e))
    d = opt.state_dict()
    assert d['clip_threshold'] == 0.0 and d['average_accumulated'] is False


def test_averaging_scales_the_accumulated_gradient():
    batches = [_image(0), _image(1)]
    model, chain, opt = _setup(average_accumulated=True)
    p0, v0 = (t.cpu().numpy() for t in _state(model))
    opt.accumulate(chain, *batches[0], 1.0)
    opt.update(chain, *batches[1], 1.0)
    model_e, chain_e, _ = _setup()
    g0, g1 = _gradient(chain_e, batches[0]), _gradient(chain_e, batches[1])
    want_p, want_v = _np_update(p0, g0.cpu().numpy(), g1.cpu().numpy(), v0, LR, 0.5)
    got = _state(model)
    assert _np_bits_equal(got[0].cpu().numpy(), want_p) and _np_bits_equal(got[1].cpu().numpy(), want_v)


def test_device_lr_path_has_the_bits_of_the_ordinary_step():
    batch = _image(0)
    res = []
    for device_lr in (False, True):
        model, chain, opt = _setup(device_lr=device_lr)
        kernels = []
        inner, inner_h = ops.sgd_momentum_wd, ops.sgd_momentum_wd_hyper
        ops.sgd_momentum_wd = lambda *a, **k: (kernels.append('plain'), inner(*a, **k))[1]
        ops.sgd_momentum_wd_hyper = lambda *a, **k: (kernels.append('hyper'), inner_h(*a, **k))[1]
        try:
            for i in range(3):
                opt.lr = LR * (i + 1)
                opt.update(chain, *batch, 1.0)
        finally:
            ops.sgd_momentum_wd, ops.sgd_momentum_wd_hyper = inner, inner_h
        assert kernels == ['hyper' if device_lr else 'plain'] * 3
        res.append(_state(model))
    _assert_same_state(*res)


def test_clipping():
    batch = _image(0)
    model, chain, opt = _setup()
    p0, v0 = (t.cpu().numpy() for t in _state(model))
    g = _gradient(chain, batch)                     # (does not move the parameters; the models below replay the same first step)
    norm64 = float(np.sqrt(np.sum(g.cpu().numpy().astype(np.float64) ** 2)))
    assert np.isfinite(norm64) and norm64 > 0
    # plain
    model_a, chain_a, opt_a = _setup()
    for _ in range(3):
        opt_a.update(chain_a, *batch, 1.0)
    # a threshold the norm never reaches: the same bits
    model_b, chain_b, opt_b = _setup()
    opt_b.add_hook(GradientClipping(1e30))
    norms = []
    for _ in range(3):
        opt_b.update(chain_b, *batch, 1.0)
        norms.append(float(opt_b.grad_norm))
    _assert_same_state(_state(model_a), _state(model_b))
    print('grad_norm', norms[0], 'float64 norm of the cloned gradient', norm64)
    assert _ulp_apart(norms[0], F(norm64)) <= 1 and int(opt_b.skipped_updates) == 0
    # half the norm: the restatement with scale = threshold / norm in float32
    model_c, chain_c, opt_c = _setup()
    thr = norm64 / 2
    opt_c.add_hook(GradientClipping(thr))
    opt_c.update(chain_c, *batch, 1.0)
    norm = F(float(opt_c.grad_norm))
    assert _ulp_apart(norm, F(norm64)) <= 1
    scale = F(1.0) * (F(thr) / norm)
    want_p, want_v = _np_update(p0, None, g.cpu().numpy(), v0, LR, scale)
    got = _state(model_c)
    assert _np_bits_equal(got[0].cpu().numpy(), want_p) and _np_bits_equal(got[1].cpu().numpy(), want_v)
    d = opt_c.state_dict()
    assert d['clip_threshold'] == thr
    model_d, chain_d, opt_d = _setup()
    opt_d.load_state_dict(d)
    assert opt_d.clip_threshold == thr and opt_d.average_accumulated is False
    d.pop('clip_threshold'), d.pop('average_accumulated')           # a file from before the keys existed
    opt_d.load_state_dict(d)
    assert opt_d.clip_threshold == 0.0


def test_data_parallel_accumulation_reduces_once_per_bucket(tmp_path):
    batches = [_image(0), _image(1)]
    model, chain, opt = _setup()
    for _ in range(2):
        opt.accumulate(chain, *batches[0], 1.0)
        opt.update(chain, *batches[1], 1.0)
    want = _state(model)
    torch.distributed.init_process_group('gloo', init_method='file://' + str(tmp_path / 'store'), rank=0, world_size=1)
    try:
        model, chain, opt = _setup()
        opt.enable_data_parallel(bucket_bytes=1 << 20, sync_single_rank=True)
        assert opt.sync.active and len(opt.sync.buckets) > 3
        calls = []
        inner = opt.sync._all_reduce
        opt.sync._all_reduce = lambda sl: (calls.append(sl.numel()), inner(sl))[1]
        for _ in range(2):
            opt.accumulate(chain, *batches[0], 1.0)
            assert calls == [] and opt.sync.before_bucket is None and chain.grad_ready_hook is not None
            opt.update(chain, *batches[1], 1.0)
            assert len(calls) == len(opt.sync.buckets) and sum(calls) == model.ps.grads.numel()
            assert opt.sync.before_bucket is None
            calls.clear()
        _assert_same_state(want, _state(model))
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize('clip', [False, True], ids=['device_lr', 'clipping'])
def test_graphed_step_follows_the_learning_rate_without_capturing_again(clip, monkeypatch):
    """Three warm-up steps at the first learning rate, then five with the learning rate changed between them: replays of the ONE capture
    against eager updates (the layout of tests/test_freeze_gpu.py: the sampler state of a captured step cannot be rewound)."""
    batch = _image(0)
    lrs = [LR * 0.5, LR * 2, LR * 2, LR * 0.1, LR]
    threshold = 1e-2            # far below the gradient norm of a freshly initialised detector: every step is clipped
    captures = []
    inner = GraphedStep._capture
    monkeypatch.setattr(GraphedStep, '_capture', lambda self: (captures.append(1), inner(self))[1])
    res = []
    for graphed in (False, True):
        model, chain, opt = _setup(device_lr=not clip, high_priority_stream=False)
        if clip:
            opt.add_hook(GradientClipping(threshold))
        if graphed:
            step = GraphedStep(opt, chain, batch, 1.0, warmup=3)
            for lr in lrs:
                opt.lr = lr
                step(*batch)
            assert captures == [1]              # the constructor's capture served all five learning rates
        else:
            for lr in [LR] * 3 + lrs:
                opt.lr = lr
                opt.update(chain, *batch, 1.0)
        res.append(_state(model) + ((float(opt.grad_norm),) if clip else ()))
    _assert_same_state(res[0][:2], res[1][:2])
    if clip:
        assert res[0][2] == res[1][2] and res[0][2] > threshold and int(opt.skipped_updates) == 0
    # without the hyper block a changed learning rate still captures again, as before
    model, chain, opt = _setup(high_priority_stream=False)
    step = GraphedStep(opt, chain, batch, 1.0, warmup=1)
    del captures[:]
    opt.lr = LR * 0.5
    step(*batch)
    assert captures == [1]


def test_graphed_step_refuses_a_pending_accumulator():
    batch = _image(0)
    model, chain, opt = _setup(high_priority_stream=False)
    opt.accumulate(chain, *batch, 1.0)
    with pytest.raises(RuntimeError, match='pending'):
        GraphedStep(opt, chain, batch, 1.0)
    opt.update(chain, *batch, 1.0)
    step = GraphedStep(opt, chain, batch, 1.0, warmup=1)
    opt.accumulate(chain, *batch, 1.0)
    with pytest.raises(RuntimeError, match='pending'):
        step(*batch)


# ---- 3. the command line ------------------------------------------------------------------------------------------------------------------
def _args(out, iteration, extra=(), resume=''):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', str(iteration), '--batch-size', '1', '--image-size', '256', '320',
                                            '--log-interval', '1', '--snapshot-interval', '1', '--label_file', '/nonexistent', '--lr', '0.004']
                                           + list(extra) + (['--resume', resume] if resume else []))


def test_train_cli_accumulates_clips_warms_up_and_resumes_bit_identically(tmp_path):
    import train
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    flags = ['--accum-steps', '2', '--grad-clip', '10', '--warmup-iterations', '2', '--lr-steps', '3']
    train.run(_args(a, 4, flags))
    log = [json.loads(l) for l in open(os.path.join(a, 'log'))]
    assert [e['iteration'] for e in log] == [1, 2, 3, 4]
    s = LRSchedule(0.004, warmup_iterations=2, steps=(3,))
    assert [e['lr'] for e in log] == [s.lr_at(it) for it in (1, 2, 3, 4)]
    assert log[0]['lr'] < log[1]['lr'] < log[2]['lr'] and log[3]['lr'] == pytest.approx(0.0004)
    assert all(np.isfinite(e['main/grad_norm']) and e['main/grad_norm'] > 0 for e in log)
    assert all(np.isfinite(e['main/loss']) for e in log) and 'skipped_updates' not in log[-1]
    state = torch.load(os.path.join(a, 'trainer_2.pt'), map_location='cpu', weights_only=False)
    assert state['optim'] == {'accum_steps': 2, 'grad_clip': 10.0, 'schedule': s.describe()}
    assert state['optimizer']['clip_threshold'] == 10.0
    with pytest.raises(ValueError, match='optimizer recipe'):
        train.run(_args(b, 4, ['--accum-steps', '4'] + flags[2:], resume=os.path.join(a, 'trainer_2.pt')))
    train.run(_args(b, 4, flags, resume=os.path.join(a, 'trainer_2.pt')))
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    z2 = np.load(os.path.join(a, 'model_2.npz'))
    assert not np.array_equal(z2['head/fc2/W'], za['head/fc2/W'])
