"""Frozen-BatchNorm fine-tuning on the device (MaskRCNN.freeze, csrc/bn_frozen.hip): the kernels bit for bit against a NumPy float32
restatement / the layer-by-layer sequence / the unmasked update, a frozen layer's forward against the inference layer, the whole frozen
step against the float64 oracle evaluated with running statistics (oracle/model.py: OracleStep(bn_buffers=...)), and the properties
of the recipe: frozen parameters never move, the frozen prefix takes no backward pass, graph replay, off is off, the command line."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle.model import OracleStep, D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.nn import core  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss, calc_keypoint_loss  # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay, GraphedStep  # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch  # noqa: E402
from tests import step_harness  # noqa: E402

DEV = 'cuda:0'
STAGES = (2, 1, 1, 1)
EPS = np.float32(2e-5)
LOSSES = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss')


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- 1. kernels ---------------------------------------------------------------------------------------------------------------------
def _layer(P, C, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    x = mk(P, C) * 2 + 0.5
    gamma, beta, mean, var = mk(C) * 0.5 + 1, mk(C) * 0.1, mk(C) * 0.3 + 0.4, torch.rand(C, generator=g) * 3 + 0.05
    gamma[0] = -0.75                        # a negative scale: the sign of the zeros it makes is part of the bits
    gy = mk(P, C) * 1e-3
    return x, gamma, beta, mean, var, gy


def _np_frozen_bwd(gy, yx, gamma, beta, mean, var, mode):
    """float32, in the order of the issue: a = gamma * (1 / sqrt(var + eps)); dz = gy under the mask; gx = dz * a."""
    f = np.float32
    inv = f(1.0) / np.sqrt(var + EPS)
    a = gamma * inv
    assert inv.dtype == np.float32 and a.dtype == np.float32
    if mode == 0:
        dz = gy
    else:
        y = yx if mode == 1 else gamma * ((yx - mean) * inv) + beta
        dz = np.where(y > f(0), gy, f(0))
    return dz * a, dz


# n4 = P * C / 4: 37, 2408, 4928 and 6600 (tails of one block and of several), 4096 (a multiple of the block size, the control), 1075200
# and 1080000 (more float4 than the grid's 4096 x 256 threads: the grid-stride loop wraps, with a tail); C = 24 has a channel-group
# count that does not divide the stride of either of its grids (coefficients per element instead of per thread)
SHAPES = [(37, 4), (301, 32), (77, 256), (64, 256), (1100, 24), (4200, 1024), (180000, 24)]


@pytest.mark.parametrize('P,C', SHAPES)
def test_frozen_bwd_kernel_is_bit_exact(P, C):
    x, gamma, beta, mean, var, gy = _layer(P, C, P + C)
    dx, dgamma, dbeta, dmean, dvar, dgy = (t.to(DEV) for t in (x, gamma, beta, mean, var, gy))
    y = ops.bn_infer_fwd(dx, dgamma, dbeta, dmean, dvar, None, True)
    ynp = np.maximum(gamma.numpy() * ((x.numpy() - mean.numpy()) * (np.float32(1.0) / np.sqrt(var.numpy() + EPS))) + beta.numpy(), np.float32(0))
    assert np.array_equal(y.cpu().numpy().view(np.int32), ynp.view(np.int32))      # the forward's expression, as restated
    assert 0.2 < float((y > 0).float().mean()) < 0.8
    outs = {}
    for mode in (0, 1, 2):
        yx = (None, y, dx)[mode]
        want_gx, want_dz = _np_frozen_bwd(gy.numpy(), None if yx is None else yx.cpu().numpy(), gamma.numpy(), beta.numpy(), mean.numpy(),
                                          var.numpy(), mode)
        for want_gres in (False, True):
            for aliased in (False, True):
                g_in = dgy.clone()
                gx, gres = ops.bn_frozen_bwd(g_in, dgamma, dvar, yx=yx, beta=dbeta if mode == 2 else None, mean=dmean if mode == 2 else None,
                                             relu=mode, want_gres=want_gres, out=g_in if aliased else None)
                assert (gx.data_ptr() == g_in.data_ptr()) == aliased
                assert np.array_equal(gx.cpu().numpy().view(np.int32), want_gx.view(np.int32)), (mode, want_gres, aliased)
                if want_gres:
                    assert np.array_equal(gres.cpu().numpy().view(np.int32), want_dz.view(np.int32)), (mode, aliased)
                if not aliased:
                    assert _same_bits(g_in, dgy)            # the input is only read
        outs[mode] = gx
    assert _same_bits(outs[1], outs[2])                     # the recomputed mask is the stored one
    assert not _same_bits(outs[0], outs[1])


@pytest.mark.parametrize('masked', [False, True], ids=['gy_unmasked', 'gy_masked'])
@pytest.mark.parametrize('P,C', [(37, 4), (301, 32), (1536, 256), (180000, 24)])
def test_frozen_pair_kernels_equal_the_layer_by_layer_sequence(P, C, masked):
    """relu(bn3(xa) + bn4(xb)) in one apply and both input gradients from one read of gy: the bits of
    bn_infer_fwd(xb) -> bn_infer_fwd(xa, residual, relu) and of two single-layer backward calls."""
    xa, ga, ba, ma, va, gy = (t.to(DEV) for t in _layer(P, C, 3 * P + C))
    xb, gb, bb, mb, vb, _ = (t.to(DEV) for t in _layer(P, C, 5 * P + C))
    xb = xb * 0.7 - 1.0
    r = ops.bn_infer_fwd(xb, gb, bb, mb, vb, None, False)
    y_ref = ops.bn_infer_fwd(xa, ga, ba, ma, va, r, True)
    y = ops.bn_infer_fwd_pair(xa, ga, ba, ma, va, xb, gb, bb, mb, vb)
    assert _same_bits(y, y_ref) and 0.1 < float((y > 0).float().mean()) < 0.9
    if masked:
        gy = torch.where(y_ref > 0, gy, torch.zeros_like(gy)).contiguous()
        gxa_ref, _ = ops.bn_frozen_bwd(gy, ga, va, relu=0)
        gxb_ref, _ = ops.bn_frozen_bwd(gy, gb, vb, relu=0)
    else:
        gxa_ref, g_r = ops.bn_frozen_bwd(gy, ga, va, yx=y_ref, relu=1, want_gres=True)
        gxb_ref, _ = ops.bn_frozen_bwd(g_r, gb, vb, relu=0)
    gxa, gxb = ops.bn_frozen_bwd_pair(gy, None if masked else y_ref, ga, va, gb, vb)
    assert _same_bits(gxa, gxa_ref) and _same_bits(gxb, gxb_ref)
    g_in = gy.clone()
    gxa2, gxb2 = ops.bn_frozen_bwd_pair(g_in, None if masked else y_ref, ga, va, gb, vb, out_a=g_in)      # gxa over gy
    assert gxa2.data_ptr() == g_in.data_ptr() and _same_bits(gxa2, gxa_ref) and _same_bits(gxb2, gxb_ref)
    assert torch.isfinite(gxa).all() and torch.isfinite(gxb).all() and not _same_bits(gxa, gxb)


@pytest.mark.parametrize('start,end', [(0, 64 * 50), (128, 64 * 31), (100, 2996), (64 * 7 + 4, 64 * 44 + 60), (101, 2999), (3, 70), (130, 133)],
                         ids=lambda v: str(v))
def test_masked_sgd_kernel(start, end):
    """Trainable elements: the bits of mrcnn_sgd_momentum_wd_f32; frozen blocks and everything outside the section: untouched (their
    gradient is NaN, so a kernel that read-modified-wrote them would leave NaNs)."""
    nblk, n = 50, 64 * 50
    g_ = torch.Generator(device='cpu').manual_seed(17)
    p0, g0, v0 = (torch.randn(n, generator=g_) for _ in range(3))
    frozen = torch.rand(nblk, generator=g_) < 0.4
    frozen[[0, 1, 2, 7, 46]] = torch.tensor([False, True, False, True, False])
    bits = np.zeros(64, bool)
    bits[:nblk] = frozen.numpy()
    mask = torch.from_numpy(np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view('<u4').reshape(-1).view(np.int32).copy()).to(DEV)
    elem_frozen = frozen.repeat_interleave(64)
    lr, mom, wd = 1e-2, 0.9, 5e-4
    pr, vr = p0.to(DEV), v0.to(DEV)
    ops.sgd_momentum_wd(pr, g0.to(DEV), vr, lr, mom, wd)            # the unmasked kernel on the same data, whole buffer
    g_nan = g0.clone()
    g_nan[elem_frozen] = float('nan')
    p, g, v = p0.to(DEV), g_nan.to(DEV), v0.to(DEV)
    ops.sgd_momentum_wd_masked(p[start:end], g[start:end], v[start:end], start, mask, lr, mom, wd)
    inside = torch.zeros(n, dtype=torch.bool)
    inside[start:end] = True
    upd = inside & ~elem_frozen
    assert upd.any()
    for got, ref, old in ((p, pr, p0), (v, vr, v0)):
        got, ref = got.cpu(), ref.cpu()
        assert torch.equal(_bits(got)[upd], _bits(ref)[upd])
        assert torch.equal(_bits(got)[~upd], _bits(old)[~upd])
        assert torch.isfinite(got).all()
    assert not torch.equal(_bits(p.cpu())[upd], _bits(p0)[upd])


# ---- 2. a frozen layer's forward is the inference layer ------------------------------------------------------------------------------
@pytest.mark.parametrize('relu,residual', [(True, True), (True, False), (False, False)])
def test_frozen_layer_forward_has_the_inference_bits(relu, residual):
    P, C = 301, 32
    ps = core.ParamStore()
    bn = core.BatchNorm(ps, 'bn', C)
    ps.materialise(DEV)
    x, gamma, beta, mean, var, _ = (t.to(DEV) for t in _layer(P, C, 9))
    ps.p('bn/gamma').copy_(gamma)
    ps.p('bn/beta').copy_(beta)
    ps.buffers['bn/avg_mean'].copy_(mean)
    ps.buffers['bn/avg_var'].copy_(var)
    x = x.view(1, 7, 43, C)
    res = (torch.randn(x.shape, generator=torch.Generator().manual_seed(1)).to(DEV)) if residual else None
    want = ops.bn_infer_fwd(x, gamma, beta, mean, var, res, relu)
    assert core.TRAIN
    bn.frozen = True
    y, ctx = bn.fwd(x, relu=relu, residual=res)
    assert _same_bits(y, want)
    assert ctx[0] == 'frozen' and len(ctx) == 2 and (ctx[1] is y if relu else ctx[1] is None)       # y or nothing: no mean / invstd
    assert _same_bits(ps.buffers['bn/avg_mean'], mean) and _same_bits(ps.buffers['bn/avg_var'], var)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    gx, gres = bn.bwd(ctx, gy, want_gres=relu)
    want_gx, want_dz = _np_frozen_bwd(gy.cpu().numpy(), y.cpu().numpy(), gamma.cpu().numpy(), None, None, var.cpu().numpy(), 1 if relu else 0)
    assert np.array_equal(gx.cpu().numpy().view(np.int32), want_gx.view(np.int32))
    assert gres is None if not relu else np.array_equal(gres.cpu().numpy().view(np.int32), want_dz.view(np.int32))
    assert not ps.grads.any()                               # no gradient of gamma / beta
    bn.frozen = False
    y2, ctx2 = bn.fwd(x, relu=relu, residual=res)           # back to batch statistics
    assert len(ctx2) == 5 and not _same_bits(y2, want)


# ---- 3. the whole frozen step against the oracle --------------------------------------------------------------------------------------
_grad_ok, _seeded = step_harness.grad_ok, step_harness.seed


def _build(kind, seed=None):
    if kind == 'mask':
        m = MaskRCNN(n_fg_class=80, device=DEV, seed=7 if seed is None else seed, _test_shrink=dict(stages=STAGES, width_div=2))
        chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, mask_rows='positives')
        b = make_batch(3, 2, 128, 160, G=3)
        key, stages, okw = 'masks', STAGES, {}
    else:
        K, NMC = 17, 2
        m = MaskRCNN(n_fg_class=1, n_keypoints=K, n_mask_convs=NMC, head_arch='fpn_keypoint', device=DEV, seed=11 if seed is None else seed,
                     _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2))
        chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_keypoint_loss, binary_mask=False)
        b = make_batch(5, 2, 128, 160, G=3, n_fg_class=1, n_keypoints=K)
        key, stages, okw = 'keypoints', (1, 1, 1, 1), dict(mask_conv_names=['mask_convs/%d' % i for i in range(NMC)], n_keypoints=K)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
    b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    return m, chain, [b['imgs'], b['bboxes'], b['labels'], b[key]], stages, okw


def _nontrivial_norms(m, chain, batch, seed=21):
    """Affine and statistics a test can tell from fresh ones, and that fit the data: every gamma U(0.5, 1.5), every beta N(0, 0.1) from a
    fixed seed, then 30 training-mode forward calls on the test batch (decay 0.9: 0.9^30 = 4 % of the initial (0, 1) buffers is left).
    Returns the training-mode losses of the last of those calls."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    for n in m.ps.names():
        if n.endswith('/gamma'):
            m.ps.p(n).copy_(torch.rand(m.ps.p(n).shape, generator=g) + 0.5)
        elif n.endswith('/beta'):
            m.ps.p(n).copy_(torch.randn(m.ps.p(n).shape, generator=g) * 0.1)
    assert m.freeze_state == (False, 0) and core.TRAIN
    for _ in range(30):
        chain(*batch, 1.0)
    return {k: float(chain.observation[k]) for k in LOSSES}


@pytest.mark.parametrize('at', [0, 2])
@pytest.mark.parametrize('kind', ['mask', 'keypoint'])
def test_frozen_step_losses_and_gradients_match_oracle(kind, at, grad_tol=1e-3):
    m, chain, batch, stages, okw = _build(kind)
    train_losses = _nontrivial_norms(m, chain, batch)
    ps = m.ps
    buffers = {k: v.detach().cpu().clone() for k, v in ps.buffers.items()}
    assert all(float((v - (1.0 if k.endswith('avg_var') else 0.0)).abs().max()) > 1e-3 for k, v in buffers.items())
    m.freeze(bn=True, at=at)
    loss = chain(*batch, 1.0)
    loss.backward()
    torch.cuda.synchronize()
    obs = {k: float(v) for k, v in chain.observation.items()}
    print('training-mode losses', train_losses)
    print('frozen-step losses  ', {k: obs[k] for k in LOSSES})
    for k in LOSSES:        # a guard, not a measurement: the recipe above keeps the frozen network in the regime of the trained one
        assert 0.5 * train_losses[k] <= obs[k] <= 2.0 * train_losses[k], (k, obs[k], train_losses[k])
    for k, v in ps.buffers.items():
        assert _same_bits(v, buffers[k]), k                  # running statistics are constants of the frozen step
    params = {n: ps.p(n).detach().cpu().to(D).requires_grad_(True) for n in ps.names()}
    t = {k: v.cpu().numpy() for k, v in chain.targets.items() if torch.is_tensor(v)}
    t['gt_rpn_loc'], t['gt_rpn_label'] = (x.cpu().numpy() for x in chain.rpn_targets)
    t['mask_rois_xy5'], t['mask_levels'], t['mask_label'] = (x.cpu().numpy() for x in chain.mask_inputs)
    assert (t['gt_roi_label'] > 0).sum() >= 4 and (t['gt_rpn_label'] == 1).sum() >= 2      # the case exercises every loss
    oracle = OracleStep(params, stages, m.head.n_class, m.head.LOC0, bn_buffers=buffers, **okw)
    img4 = torch.cat([batch[0].cpu().permute(0, 2, 3, 1), torch.zeros((2, 128, 160, 1))], -1).to(D)
    out = oracle.losses(img4, t)
    for k in LOSSES:
        want = float(out[k].detach())
        print(k, obs[k], want)
        assert abs(obs[k] - want) <= 1e-4 * max(abs(want), 1e-3), (k, obs[k], want)
    sum(out[k] for k in LOSSES).backward()
    from oracle import model as om
    om.set_dtype(torch.float32)             # the float32 noise floor of this network: the same oracle step in float32
    try:
        p32 = {n: ps.p(n).detach().cpu().requires_grad_(True) for n in ps.names()}
        out32 = OracleStep(p32, stages, m.head.n_class, m.head.LOC0, bn_buffers=buffers, **okw).losses(img4.float(), t)
        sum(out32[k] for k in LOSSES).backward()
    finally:
        om.set_dtype(torch.float64)
    frozen = ps.frozen
    assert all(n in frozen for n in ps.names() if '/resnet/' in n and n.rsplit('/', 1)[1] in ('gamma', 'beta'))
    assert ('extractor/resnet/res2/a/conv1/W' in frozen) == (at == 2) and 'extractor/resnet/res3/a/conv1/W' not in frozen
    gmax = max(float(params[n].grad.abs().max()) for n in ps.names() if n not in frozen and params[n].grad is not None)
    worst = 0.0
    for n in ps.names():
        if n in frozen:                     # constants: no gradient is computed (the oracle's, for stem / res2, is not compared)
            assert not ps.g(n).any(), n
            continue
        want = params[n].grad if params[n].grad is not None else torch.zeros_like(params[n])
        w32 = p32[n].grad if p32[n].grad is not None else torch.zeros_like(p32[n])
        got = ps.g(n).cpu().to(D)
        scale = max(float(want.abs().max()), 1e-3 * gmax)
        err = float((got - want).abs().max()) / scale
        floor = float((w32.to(D) - want).abs().max()) / scale
        worst = max(worst, err)
        assert _grad_ok(got, want, err, floor, grad_tol), (n, err, floor)
    print('worst relative gradient error', worst)


# ---- 4. frozen means frozen -----------------------------------------------------------------------------------------------------------
def _is_prefix(n):
    return any(n.startswith('extractor/resnet/' + s) for s in ('conv1/', 'bn1/', 'res2/'))


def test_frozen_parameters_do_not_move():
    res = []
    for sectioned in (False, True):
        m, chain, batch, _, _ = _build('mask')
        _nontrivial_norms(m, chain, batch)
        _seeded(chain)
        m.freeze(True, 2)
        ps = m.ps
        ps.momentum.copy_(torch.randn(ps.momentum.shape, generator=torch.Generator().manual_seed(4)) * 1e-4)     # a momentum to decay
        p0, v0 = ps.params.clone(), ps.momentum.clone()
        b0 = {k: v.clone() for k, v in ps.buffers.items()}
        opt = MomentumSGD(lr=1e-2, momentum=0.9, sectioned_update=sectioned).setup(chain)
        opt.LOCAL_BUCKET_BYTES = 256 << 10
        opt.add_hook(WeightDecay(5e-4))
        calls = []
        inner = opt._sgd_section

        def spy(start, end, inner=inner, calls=calls):
            calls.append((start, end))
            inner(start, end)
        opt._sgd_section = spy
        for _ in range(3):
            opt.update(chain, *batch, 1.0)
        torch.cuda.synchronize()
        assert bool(calls) == sectioned and all(s % 64 == 0 for s, _ in calls)
        n_frozen = n_moved = 0
        for n in ps.names():
            o, shape = ps.offsets[n]
            sl = slice(o, o + int(np.prod(shape)))
            if n.rsplit('/', 1)[1] in ('gamma', 'beta') and '/resnet/' in n or _is_prefix(n):
                assert n in ps.frozen
                assert _same_bits(ps.params[sl], p0[sl]) and _same_bits(ps.momentum[sl], v0[sl]), n
                assert not ps.grads[sl].any(), n
                n_frozen += 1
            else:
                assert n not in ps.frozen
                assert not _same_bits(ps.momentum[sl], v0[sl]), n
                if n.endswith('/W'):
                    assert not _same_bits(ps.params[sl], p0[sl]), n
                    n_moved += 1
        assert n_frozen >= 40 + 8 and n_moved >= 20
        for k, v in ps.buffers.items():
            assert _same_bits(v, b0[k]), k
        assert torch.isfinite(ps.params).all()
        res.append((ps.params.clone(), ps.momentum.clone(), float(chain.observation['loss'])))
    assert res[0][2] == res[1][2]
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])       # sectioned = single pass, frozen too


# ---- 5. the prefix is really skipped --------------------------------------------------------------------------------------------------
def test_frozen_prefix_takes_no_backward_pass():
    m, chain, batch, _, _ = _build('mask')
    _nontrivial_norms(m, chain, batch)
    m.freeze(True, 2)
    ps = m.ps
    sentinel = 1234.5
    for n in ps.names():
        if _is_prefix(n):
            ps.g(n).fill_(sentinel)
    seen = []
    chain.grad_ready_hook = seen.append
    loss = chain(*batch, 1.0)
    tape = m.extractor.tape
    taped = [b for b, _ in tape['blocks']]
    assert [b.conv1.name.split('/')[2:4] for b in taped] == [['res3', 'a'], ['res4', 'a'], ['res5', 'a']]
    assert all(ctx is not None and ctx[0] == 'frozen' for _, ctx in tape['blocks'])
    assert tape['conv1'] is None and tape['bn1'] is None and 'pool_in' not in tape
    loss.backward()
    torch.cuda.synchronize()
    chain.grad_ready_hook = None
    for n in ps.names():
        if _is_prefix(n):
            assert bool((ps.g(n) == sentinel).all()), n                 # never written
        elif n not in ps.frozen:
            assert torch.isfinite(ps.g(n)).all(), n
            if n.endswith('/W') and '/resnet/' in n:
                assert ps.g(n).any(), n                                     # the trained stages above it do take theirs
    # every prefix is still reported, in descending order down to 0: buckets and sections close as without freezing
    assert seen == sorted(seen, reverse=True) and seen[-1] == 0
    for name in ('extractor/resnet/res3/a/conv1', 'extractor/resnet/res2/b1/conv1', 'extractor/resnet/res2/a/conv1'):
        assert min(o for n, (o, _) in ps.offsets.items() if n.startswith(name)) in seen, name


@pytest.mark.parametrize('at', [1, 2, 3, 4, 5])
def test_every_prefix_leaves_the_trained_layers_their_gradients(at):
    """freeze_at changes what is computed, not what the trained layers get: the forward pass is the same, so every parameter that is
    still trained has the gradient bits of the freeze_bn-only step on the same batch and samples; the prefix's slots hold zeros; the
    tape holds exactly the trained blocks."""
    m, chain, batch, _, _ = _build('mask')
    _nontrivial_norms(m, chain, batch)
    grads, losses = [], []
    for k in (0, at):
        m.freeze(True, k)
        _seeded(chain)
        loss = chain(*batch, 1.0)
        n_taped = len(m.extractor.tape['blocks'])
        loss.backward()
        torch.cuda.synchronize()
        grads.append(m.ps.grads.clone())
        losses.append(float(loss.detach()))
    assert n_taped == sum(STAGES[max(at - 1, 0):])
    assert losses[0] == losses[1]
    ps = m.ps
    prefixes = tuple(p + '/' for p in m.extractor.frozen_prefixes())
    assert len(prefixes) == 2 + sum(STAGES[:at - 1])
    checked = 0
    for n in ps.names():
        o, shape = ps.offsets[n]
        sl = slice(o, o + int(np.prod(shape)))
        if n in ps.frozen:
            assert n.startswith(prefixes) or n.rsplit('/', 1)[1] in ('gamma', 'beta'), n
            assert not grads[1][sl].any(), n
        else:
            assert not n.startswith(prefixes)
            assert _same_bits(grads[1][sl], grads[0][sl]), n
            checked += 1
    assert checked >= 20 and 'extractor/toplayer/W' not in ps.frozen and 'extractor/lat_p2/W' not in ps.frozen


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------------------
def test_graphed_frozen_step_replays_the_eager_step():
    res = []
    for graphed in (False, True):
        m, chain, batch, _, _ = _build('mask')
        _nontrivial_norms(m, chain, batch)
        _seeded(chain)
        m.freeze(True, 2)
        opt = MomentumSGD(lr=1e-2, momentum=0.9, high_priority_stream=False).setup(chain)
        opt.add_hook(WeightDecay(0.0005))
        if graphed:
            g = GraphedStep(opt, chain, batch, 1.0, warmup=3)
            for _ in range(2):
                g(*batch)
        else:
            for _ in range(5):
                opt.update(chain, *batch, 1.0)
        torch.cuda.synchronize()
        res.append((m.ps.params.clone(), m.ps.momentum.clone(), float(chain.observation['loss'])))
    assert res[0][2] == res[1][2]
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])


# ---- 7. off is off --------------------------------------------------------------------------------------------------------------------
def test_unfreezing_gives_back_the_ordinary_step():
    res = []
    for was_frozen in (False, True):
        m, chain, batch, _, _ = _build('mask')
        opt = MomentumSGD(lr=1e-2, momentum=0.9).setup(chain)
        opt.add_hook(WeightDecay(0.0005))
        if was_frozen:
            m.freeze(True, 2)
            _seeded(chain)
            chain(*batch, 1.0).backward()               # a frozen step in between (no update: the two models stay equal)
            m.freeze(False, 0)
            assert m.ps.frozen_mask is None and not m.ps.frozen and m.freeze_state == (False, 0)
        _seeded(chain)
        kernels = []
        inner, inner_masked = ops.sgd_momentum_wd, ops.sgd_momentum_wd_masked
        ops.sgd_momentum_wd = lambda *a, **k: (kernels.append('plain'), inner(*a, **k))[1]
        ops.sgd_momentum_wd_masked = lambda *a, **k: (kernels.append('masked'), inner_masked(*a, **k))[1]
        try:
            opt.update(chain, *batch, 1.0)
        finally:
            ops.sgd_momentum_wd, ops.sgd_momentum_wd_masked = inner, inner_masked
        torch.cuda.synchronize()
        assert kernels == ['plain']
        assert not any(n.frozen for bl in m.extractor.stages for b in bl for n in b.norms()) and not m.extractor.bn1.frozen
        res.append((float(chain.observation['loss']), m.ps.grads.clone(), m.ps.params.clone(), m.ps.momentum.clone(),
                    {k: v.clone() for k, v in m.ps.buffers.items()}))
    assert res[0][0] == res[1][0]
    for i in (1, 2, 3):
        assert _same_bits(res[0][i], res[1][i])
    for k in res[0][4]:
        assert _same_bits(res[0][4][k], res[1][4][k]), k


def test_freeze_argument_errors():
    m, chain, batch, _, _ = _build('mask')
    with pytest.raises(ValueError):
        m.freeze(bn=False, at=2)
    with pytest.raises(ValueError):
        m.freeze(bn=True, at=6)
    assert m.freeze_state == (False, 0) and m.ps.frozen_mask is None


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------------
def _args(out, iteration, extra=(), resume=''):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', str(iteration), '--batch-size', '1', '--image-size', '256', '320',
                                            '--log-interval', '1', '--snapshot-interval', '1', '--label_file', '/nonexistent']
                                           + list(extra) + (['--resume', resume] if resume else []))


def test_train_cli_freezes_and_resumes_bit_identically(tmp_path, capsys):
    import train
    w, a, b = str(tmp_path / 'w'), str(tmp_path / 'a'), str(tmp_path / 'b')
    flags = ['--freeze-bn', '1', '--freeze-at', '2']
    train.run(_args(str(tmp_path / 'n'), 0, flags))
    assert 'freshly initialised BatchNorm statistics' in capsys.readouterr().out          # no --weight / --resnet50-npz / --resume: warned
    # a backbone whose running statistics fit the data, as an imported one's do: 20 ordinary iterations (0.9^20 = 12 % of the initial
    # (0, 1) buffers is left) - frozen on the fresh buffers the full-depth network's activations explode (losses of 1e35)
    train.run(_args(w, 20, ['--snapshot-interval', '20']))
    flags += ['--weight', os.path.join(w, 'model_20.npz')]
    capsys.readouterr()
    train.run(_args(a, 3, flags))
    assert 'freshly initialised' not in capsys.readouterr().out
    log = [json.loads(l) for l in open(os.path.join(a, 'log'))]
    assert [e['iteration'] for e in log] == [1, 2, 3]
    print([e['main/loss'] for e in log])
    # (1e3: two orders above the O(1 - 10) of these losses at initialisation - ln 81 = 4.4 for the class loss - and 32 below the explosion)
    assert all(np.isfinite(e['main/' + k]) and e['main/' + k] < 1e3 for e in log for k in ('loss',) + LOSSES)
    state = torch.load(os.path.join(a, 'trainer_2.pt'), map_location='cpu', weights_only=False)
    assert state['freeze'] == {'bn': 1, 'at': 2}
    z1, z3 = np.load(os.path.join(a, 'model_1.npz')), np.load(os.path.join(a, 'model_3.npz'))
    moved = [k for k in z1.files if not np.array_equal(z1[k], z3[k])]
    assert 'head/fc2/W' in moved and 'extractor/resnet/res3/a/conv1/W' in moved
    assert not [k for k in moved if '/resnet/res2/' in k or '/resnet/conv1/' in k or '/bn' in k], moved
    with pytest.raises(ValueError, match='freezing'):
        train.run(_args(b, 3, resume=os.path.join(a, 'trainer_2.pt')))                      # other settings: refused
    train.run(_args(b, 3, flags, resume=os.path.join(a, 'trainer_2.pt')))
    zb = np.load(os.path.join(b, 'model_3.npz'))
    assert sorted(zb.files) == sorted(z3.files) and len(z3.files) > 100
    for k in z3.files:
        np.testing.assert_array_equal(z3[k], zb[k], err_msg=k)
