"""GPU tests of GroupNorm in the RoI heads (csrc/groupnorm.hip, nn/core.py GroupNorm, FPNRoIMaskHead(norm='gn')):
the kernels against the float64 reference of tests/groupnorm_reference.py at the BatchNorm bars of tests/test_nn_gpu.py, the bitwise
properties of the backward, the heads against float64 autograd on the CPU, the whole training step, inference, and the untouched
defaults."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'chainer-maskrcnn_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_keypoint_loss  # noqa: E402
from chainer_maskrcnn.model.head.fpn_roi_mask_head import FPNRoIMaskHead, roi_align_fpn_fwd, roi_align_fpn_bwd  # noqa: E402
from chainer_maskrcnn.model.head.fpn_roi_keypoint_head import FPNRoIKeypointHead  # noqa: E402
from chainer_maskrcnn.nn import core  # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay  # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch  # noqa: E402
import groupnorm_reference as gnr  # noqa: E402
from tests import step_harness  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
D = torch.float64


def _rel(got, ref):
    """The metric of tests/test_nn_gpu.py."""
    ref = torch.as_tensor(ref, dtype=D)
    return (got.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _cap(C, Cp, G):
    """The largest H * W of the register-resident path for this channel geometry, by bisection on the plan query."""
    lo, hi = 1, 1 << 20
    assert ops.group_norm_plan(1, 1, lo, C, Cp, G)[0] == 0 and ops.group_norm_plan(1, 1, hi, C, Cp, G)[0] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.group_norm_plan(1, 1, mid, C, Cp, G)[0] == 0 else (lo, mid)
    return lo


# (R, H, W, C, Cp, G), the path the plan query must report; W = 'cap' / 'cap+1': H * W at / above the register path's cap, found by bisection
CASES = [((1, 1, 1, 32, 32, 32), 0),            # one element per group: y = beta and gx = 0 exactly
         ((3, 7, 7, 64, 64, 32), 0),            # cpg 2: a float4 straddles two groups
         ((2, 14, 14, 256, 256, 32), 0),        # the production slabs
         ((5, 7, 7, 256, 256, 32), 0),
         ((2, 5, 3, 96, 96, 32), 1),            # cpg 3: generic
         ((2, 4, 4, 48, 64, 16), 1),            # padded channels, cpg 3
         ((2, 4, 4, 48, 64, 12), 0),            # padded channels on the register path (cpg 4)
         ((2, 33, 31, 64, 64, 32), 1),          # above the cap
         ((2, 1, 'cap', 64, 64, 32), 0),        # exactly at the cap
         ((2, 1, 'cap+1', 64, 64, 32), 1),      # one above
         ((2, 10, 10, 64, 64, 32), 0),          # four pixels per thread (the kernels are built for 2, 4 and 8)
         ((2, 6, 5, 96, 96, 8), 0),             # cpg 12: three float4 columns per workgroup, LDS-only reduction
         ((3, 7, 7, 128, 128, 2), 0),           # cpg 64: sixteen columns, one group per workgroup
         ((2, 3, 3, 20, 32, 20), 0)]            # cpg 1 with padding: a float4 straddles four groups
IDS = ['x'.join(map(str, c)) for c, _ in CASES]


def _resolve(case):
    R, H, W, C, Cp, G = case
    if isinstance(W, str):
        W = _cap(C, Cp, G) + (1 if W == 'cap+1' else 0)
    return (R, H, W, C, Cp, G)


def _data(case, seed=0, offset=3.0, scale=2.0):
    R, H, W, C, Cp, G = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, H, W, Cp), generator=g) * scale + offset      # (the padding carries data too: the kernels must not let it through)
    gy = torch.randn((R, H, W, Cp), generator=g)
    gamma, beta = torch.zeros(Cp), torch.zeros(Cp)
    gamma[:C] = torch.randn(C, generator=g) * 0.5 + 1.0
    beta[:C] = torch.randn(C, generator=g) * 0.5
    return x, gy, gamma, beta


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


@pytest.mark.parametrize('case,path', CASES, ids=IDS)
def test_kernels_match_the_float64_reference(case, path):
    case = _resolve(case)
    R, H, W, C, Cp, G = case
    assert ops.group_norm_plan(*case)[0] == path
    x, gy, gamma, beta = _data(case)
    xd, gyd, gd, bd = _dev(x, gy, gamma, beta)
    xr = x.clone()
    xr[..., C:] = 0
    for relu in (False, True):
        y, mean, rstd = ops.group_norm_fwd(xd, gd, bd, C, G, relu=relu)
        yr, mr, rr = gnr.group_norm_fwd(xr.numpy(), gamma.numpy(), beta.numpy(), C, G, relu=relu)
        errs = {'y': _rel(y, yr), 'mean': _rel(mean, mr), 'rstd': _rel(rstd, rr)}
        print(case, 'relu', relu, 'fwd', errs)
        assert errs['y'] <= 1e-5 and errs['mean'] <= 1e-5 and errs['rstd'] <= 1e-5, errs
        assert not y[..., C:].any()                                             # exact zeros on the padding
        y2, m2, r2 = ops.group_norm_fwd(xd, gd, bd, C, G, relu=relu, want_stats=False)
        assert m2 is None and r2 is None and torch.equal(y, y2)
        # backward: the reference takes its ReLU mask from the device's y > 0
        gg0 = torch.full((Cp,), 7.0, device=DEV)
        gb0 = torch.full((Cp,), -7.0, device=DEV)
        gx, gg, gb = ops.group_norm_bwd(gyd, xd, gd, bd, mean, rstd, C, G, relu=relu, gg=gg0, gb=gb0)
        mask = (y > 0).cpu().numpy() if relu else None
        gyr = gy.clone()
        gyr[..., C:] = 0
        gxr, ggr, gbr = gnr.group_norm_bwd(gyr.numpy(), xr.numpy(), gamma.numpy(), mr, rr, C, G, mask=mask)
        errs = {'gx': _rel(gx, gxr), 'ggamma': _rel(gg, ggr), 'gbeta': _rel(gb, gbr)}
        print(case, 'relu', relu, 'bwd', errs)
        assert errs['gx'] <= 2e-5 and errs['ggamma'] <= 2e-5 and errs['gbeta'] <= 2e-5, errs
        assert not gx[..., C:].any() and not gg[C:].any() and not gb[C:].any()
    if H * W == 1 and C == G:
        y, mean, rstd = ops.group_norm_fwd(xd, gd, bd, C, G)
        gx, _, _ = ops.group_norm_bwd(gyd, xd, gd, bd, mean, rstd, C, G)
        assert torch.equal(y, bd.expand_as(y)) and not gx.any()


def test_both_paths_are_exercised():
    paths = {ops.group_norm_plan(*_resolve(c))[0] for c, _ in CASES}
    assert paths == {0, 1} and all(ops.group_norm_plan(*_resolve(c))[0] == p for c, p in CASES)
    assert _cap(256, 256, 32) >= 196 and ops.group_norm_plan(2, 14, 14, 256, 256, 32)[0] == 0


def test_empty_batch():
    x = torch.zeros((0, 7, 7, 64), device=DEV)
    gamma, beta = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    y, mean, rstd = ops.group_norm_fwd(x, gamma, beta, 64, 32, relu=True)
    assert y.shape == (0, 7, 7, 64) and mean.shape == (0, 32) and rstd.shape == (0, 32)
    gx, gg, gb = ops.group_norm_bwd(x, x, gamma, beta, mean, rstd, 64, 32)
    assert gx.shape == (0, 7, 7, 64) and not gg.any() and not gb.any()
    keep = torch.full((64,), 2.0, device=DEV)
    ops.group_norm_bwd(x, x, gamma, beta, mean, rstd, 64, 32, gg=keep, gb=keep.clone(), accumulate_params=True)
    assert torch.equal(keep, torch.full((64,), 2.0, device=DEV))


def test_large_mean_keeps_its_digits():
    """x = randn + 100: the variance about the mean stays accurate, E[x^2] - E[x]^2 in float32 would not (3.4e-3 and more on y, rstd, gx,
    ggamma in a float32 simulation; the two-pass arithmetic at most 5.6e-5).  The bar for every quantity is 5e-4."""
    case = (2, 14, 14, 256, 256, 32)
    R, H, W, C, Cp, G = case
    x, gy, gamma, beta = _data(case, seed=1, offset=100.0, scale=1.0)
    xd, gyd, gd, bd = _dev(x, gy, gamma, beta)
    y, mean, rstd = ops.group_norm_fwd(xd, gd, bd, C, G, relu=True)
    gx, gg, gb = ops.group_norm_bwd(gyd, xd, gd, bd, mean, rstd, C, G, relu=True)
    yr, mr, rr = gnr.group_norm_fwd(x.numpy(), gamma.numpy(), beta.numpy(), C, G, relu=True)
    gxr, ggr, gbr = gnr.group_norm_bwd(gy.numpy(), x.numpy(), gamma.numpy(), mr, rr, C, G, mask=(y > 0).cpu().numpy())
    errs = {'y': _rel(y, yr), 'mean': _rel(mean, mr), 'rstd': _rel(rstd, rr), 'gx': _rel(gx, gxr), 'ggamma': _rel(gg, ggr), 'gbeta': _rel(gb, gbr)}
    print('large mean', errs)
    assert all(e <= 5e-4 for e in errs.values()), errs


@pytest.mark.parametrize('case', [(3, 14, 14, 256, 256, 32), (3, 7, 7, 64, 64, 32), (2, 5, 3, 96, 96, 32), (2, 4, 4, 48, 64, 16)],
                         ids=['register_cpg8', 'register_cpg2', 'generic', 'generic_padded'])
def test_backward_bitwise_properties(case):
    R, H, W, C, Cp, G = case
    x, gy, gamma, beta = _data(case, seed=2)
    x[..., C:] = 0
    gy[..., C:] = 0
    xd, gyd, gd, bd = _dev(x, gy, gamma, beta)
    y, mean, rstd = ops.group_norm_fwd(xd, gd, bd, C, G, relu=True)
    a = ops.group_norm_bwd(gyd, xd, gd, bd, mean, rstd, C, G, relu=True)
    b = ops.group_norm_bwd(gyd, xd, gd, bd, mean, rstd, C, G, relu=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))                          # the same bits on every run
    masked = (gyd * (y > 0)).contiguous()
    c = ops.group_norm_bwd(masked, xd, gd, bd, mean, rstd, C, G, relu=False)
    assert all(torch.equal(p, q) for p, q in zip(a, c))                          # the recomputed mask is the forward's y > 0
    g = torch.Generator().manual_seed(3)
    pre_g, pre_b = _dev(torch.randn(Cp, generator=g), torch.randn(Cp, generator=g))
    gg, gb = pre_g.clone(), pre_b.clone()
    gx, _, _ = ops.group_norm_bwd(gyd, xd, gd, bd, mean, rstd, C, G, relu=True, gg=gg, gb=gb, accumulate_params=True)
    assert torch.equal(gx, a[0])
    for got, pre, over in ((gg, pre_g, a[1]), (gb, pre_b, a[2])):
        want = pre + over
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float('inf'))) - want.abs()
        assert bool(((got - want).abs() <= ulp).all())


# ---- heads against float64 autograd on the CPU -----------------------------------------------------------------------------------------------
C_HEAD, FC_HEAD, GROUPS = 64, 256, 32           # the _test_shrink width (width_div 4): 32 groups of 2
SCALES = [1 / 4., 1 / 8., 1 / 16., 1 / 32.]


def _head(kind, seed=3):
    if kind == 'keypoint':
        head = FPNRoIKeypointHead(2, 5, roi_size_box=7, roi_size_mask=14, n_mask_convs=8, mask_initialW=0.01, in_channels=C_HEAD,
                                  fc_channels=FC_HEAD, norm='gn', gn_groups=GROUPS)
    else:
        head = FPNRoIMaskHead(5, roi_size_box=7, roi_size_mask=14, mask_initialW=0.01, in_channels=C_HEAD, fc_channels=FC_HEAD, norm='gn',
                              gn_groups=GROUPS)
    ps = head.ps.materialise(torch.device(DEV), seed)
    g = torch.Generator().manual_seed(seed)
    for n in ps.names():            # biases, gamma and beta away from their 0 / 1 initial values (logical channels only)
        p = ps.p(n)
        if n.endswith('/gn/gamma') or n.endswith('/gn/beta') or n == head.deconv_b or (n.endswith('/b') and p.numel() == C_HEAD):
            p += (torch.randn(p.shape, generator=g) * 0.2).to(DEV)
    ps.p(head.conv2.name + '/b')[:head.mask_out_channels] += 0.1
    return head


def _inputs(seed=4, R=12):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((2, h, w, C_HEAD), generator=g).to(DEV) for h, w in ((16, 20), (8, 10), (4, 5), (2, 3))]
    y1, x1 = torch.rand(R, generator=g) * 30, torch.rand(R, generator=g) * 40
    hh, ww = 8 + torch.rand(R, generator=g) * 26, 8 + torch.rand(R, generator=g) * 32
    idx = torch.randint(0, 2, (R,), generator=g).float()
    rois = torch.stack([idx, x1, y1, x1 + ww, y1 + hh], 1).to(DEV).contiguous()
    levels = torch.randint(0, 4, (R,), generator=g).to(torch.int32).to(DEV)
    return xs, rois, levels


def _gn_relu(h, G, gamma, beta, mask):
    """group_norm + relu; the ReLU decision is the DEVICE's y > 0 (``mask``), so a pre-activation within rounding of zero cannot decide
    the comparison either way (as in the kernel tests) - the device's y itself is compared with this function's value."""
    y = F.group_norm(h, G, gamma, beta, eps=1e-5)
    return y * mask.to(y.dtype), torch.relu(y)


def _mask_reference(head, P, pooled, masks, g_out, dtype):
    """conv2d + group_norm + relu stack, conv_transpose2d, conv2d (+ corner-aligned x2 resize) on the head's own weights in ``dtype``.
    Returns (output NCHW, the stack's relu outputs, pooled gradient NHWC, {name: parameter gradient in the store's layout})."""
    c = head.channels
    leaves = {n: P[n].to(dtype).clone().requires_grad_(True) for n in P}
    x = pooled.to(dtype).clone().requires_grad_(True)
    h, ys = x.permute(0, 3, 1, 2), []
    for cv, gn, mk in zip(head.mask_convs, head.mask_gns, masks):
        h = F.conv2d(h, leaves[cv.name + '/W'].permute(0, 3, 1, 2), leaves[cv.name + '/b'], padding=1)
        h, y = _gn_relu(h, gn.groups, leaves[gn.name + '/gamma'][:c], leaves[gn.name + '/beta'][:c], mk)
        ys.append(y.detach())
    wd = leaves[head.deconv1.name + '/W'][:, 0, 0, :c].reshape(2, 2, c, c).permute(3, 2, 0, 1)
    h = F.conv_transpose2d(h, wd, leaves[head.deconv_b], stride=2)
    K = head.mask_out_channels
    h = F.conv2d(h, leaves[head.conv2.name + '/W'][:K, 0, 0, :c][:, :, None, None], leaves[head.conv2.name + '/b'][:K])
    if head.upsample2x:
        h = F.interpolate(h, scale_factor=2, mode='bilinear', align_corners=True)
    (h * g_out.to(dtype)).sum().backward()
    return h.detach(), ys, x.grad, {n: leaves[n].grad for n in leaves}


def _box_reference(head, P, pooled, masks, g_out, dtype):
    c = head.channels
    leaves = {n: P[n].to(dtype).clone().requires_grad_(True) for n in P}
    x = pooled.to(dtype).clone().requires_grad_(True)
    h = F.conv2d(x.permute(0, 3, 1, 2), leaves[head.conv1.name + '/W'].permute(0, 3, 1, 2), leaves[head.conv1.name + '/b'], padding=1)
    h, y = _gn_relu(h, head.gn1.groups, leaves[head.gn1.name + '/gamma'][:c], leaves[head.gn1.name + '/beta'][:c], masks[0])
    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)           # the store's fc1 takes the NHWC flattening
    for fc, mk in ((head.fc1, masks[1]), (head.fc2, masks[2])):
        h = (h @ leaves[fc.name + '/W'][:, 0, 0, :].t() + leaves[fc.name + '/b']) * mk.to(dtype)
    o = h @ leaves[head.box_out.name + '/W'][:, 0, 0, :].t() + leaves[head.box_out.name + '/b']
    (o * g_out.to(dtype)).sum().backward()
    return o.detach(), [y.detach()], x.grad, {n: leaves[n].grad for n in leaves}


_check = step_harness.check


@pytest.mark.parametrize('kind,merge', [('mask', True), ('mask', False), ('keypoint', True)], ids=['mask_merged', 'mask_layerwise', 'keypoint'])
def test_mask_branch_matches_float64_autograd(kind, merge):
    head = _head(kind)
    head.merge_deconv = merge
    ps = head.ps
    xs, rois, levels = _inputs()
    assert core.TRAIN
    m = head.mask_branch(xs, rois, levels, SCALES)
    pooled = roi_align_fpn_fwd(xs, rois, levels, head.roi_size_mask, SCALES).cpu()
    tapes, td = head.mask_tape[0], head.mask_tape[1]
    assert all(nt is not None and nt[3] for _, nt in tapes) and all(t[1] is None for t, _ in tapes)     # ReLU in the GroupNorm, not in the conv
    ys_dev = [tapes[i + 1][0][0] for i in range(len(tapes) - 1)] + [td[0]]                               # each GroupNorm's output
    masks = [(y > 0).permute(0, 3, 1, 2).cpu() for y in ys_dev]
    K, S = head.mask_out_channels, head.mask_size
    g = torch.Generator().manual_seed(9)
    g_out = torch.randn((rois.shape[0], K, S, S), generator=g)
    g_mask = torch.zeros((rois.shape[0], S, S, head.conv2.cout_p))
    g_mask[..., :K] = g_out.permute(0, 2, 3, 1)
    ps.grads.zero_()
    g_pool = head.backward_mask_convs(g_mask.to(DEV).contiguous())
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    names = [n for cv, gn in zip(head.mask_convs, head.mask_gns) for n in (cv.name + '/W', cv.name + '/b', gn.name + '/gamma', gn.name + '/beta')]
    names += [head.deconv1.name + '/W', head.deconv_b, head.conv2.name + '/W', head.conv2.name + '/b']
    P = {n: ps.p(n).detach().cpu() for n in names}
    o64, y64, gp64, gr64 = _mask_reference(head, P, pooled, masks, g_out, D)
    o32, y32, gp32, gr32 = _mask_reference(head, P, pooled, masks, g_out, torch.float32)
    bad = []
    _check('output', m[..., :K].permute(0, 3, 1, 2), o64, o32, bad)
    for i, y in enumerate(ys_dev):
        _check('gn output %d' % i, y.permute(0, 3, 1, 2), y64[i], y32[i], bad)
    _check('pooled gradient', g_pool, gp64, gp32, bad)
    for n in names:
        _check(n, ps.g(n), gr64[n], gr32[n], bad)
    assert not bad, bad
    head.mask_tape = None


def test_box_branch_matches_float64_autograd():
    head = _head('mask')
    ps = head.ps
    xs, rois, levels = _inputs(seed=5)
    o = head.box_branch(xs, rois, levels, SCALES)
    pooled = roi_align_fpn_fwd(xs, rois, levels, head.roi_size_box, SCALES).cpu()
    (t1, n1), t2, t3, t4 = head.box_tape[:4]
    assert n1 is not None and n1[3] and t1[1] is None
    R = rois.shape[0]
    y_dev = t2[0].view(R, 7, 7, head.channels)
    masks = [(y_dev > 0).permute(0, 3, 1, 2).cpu(), (t3[0].view(R, -1) > 0).cpu(), (t4[0].view(R, -1) > 0).cpu()]
    g = torch.Generator().manual_seed(10)
    g_out = torch.zeros((R, head.out_p))
    g_out[:, :head.n_class] = torch.randn((R, head.n_class), generator=g)
    g_out[:, head.LOC0:head.LOC0 + 4] = torch.randn((R, 4), generator=g)
    ps.grads.zero_()
    g_feats = [torch.empty_like(x) for x in xs]
    head.backward_box(g_out.to(DEV).contiguous(), g_feats, accumulate=False)
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    names = [head.conv1.name + '/W', head.conv1.name + '/b', head.gn1.name + '/gamma', head.gn1.name + '/beta', head.fc1.name + '/W',
             head.fc1.name + '/b', head.fc2.name + '/W', head.fc2.name + '/b', head.box_out.name + '/W', head.box_out.name + '/b']
    P = {n: ps.p(n).detach().cpu() for n in names}
    o64, y64, gp64, gr64 = _box_reference(head, P, pooled, masks, g_out, D)
    o32, y32, gp32, gr32 = _box_reference(head, P, pooled, masks, g_out, torch.float32)
    bad = []
    _check('output', o, o64, o32, bad)
    _check('gn output', y_dev.permute(0, 3, 1, 2), y64[0], y32[0], bad)
    for n in names:
        _check(n, ps.g(n), gr64[n], gr32[n], bad)
    # the accumulated level gradients against the norm=None-style path: ROIAlign backward fed the reference pooled gradient
    want = {}
    for key, gp in (('f64', gp64), ('f32', gp32)):
        bufs = [torch.empty_like(x) for x in xs]
        roi_align_fpn_bwd(gp.float().to(DEV).contiguous(), bufs, rois, levels, head.roi_size_box, SCALES, accumulate=False)
        want[key] = bufs
    for l in range(len(xs)):
        _check('g_feats level %d' % l, g_feats[l], want['f64'][l].cpu(), want['f32'][l].cpu(), bad)
    assert not bad, bad


# ---- the whole step -----------------------------------------------------------------------------------------------------------------------
SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)


_build, _batch, _step = functools.partial(step_harness.build, SHRINK), step_harness.batch, step_harness.step
_predict_model = functools.partial(step_harness.predict_model, SHRINK, head_norm='gn')


def test_step_with_group_norm_is_finite_and_bit_reproducible():
    m, chain = _build(head_norm='gn')
    b = _batch()
    _step(chain, b)
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert all(np.isfinite(v) for v in obs.values()), obs
    g1 = m.ps.grads.clone()
    assert torch.isfinite(g1).all()
    gns = [n for n in m.ps.names() if '/gn/' in n]
    assert len(gns) == 10
    for n in gns:
        g = m.ps.g(n)
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, n
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)                      # no float atomics with GroupNorm on either


def test_defaults_are_untouched():
    """head_norm=None and a model built without the argument: the same parameters, the same flat gradient buffer, bit for bit."""
    res = []
    for kw in ({}, {'head_norm': None}):
        m, chain = _build(**kw)
        _step(chain, _batch())
        res.append((m.ps.params.clone(), m.ps.grads.clone(), dict(m.ps.offsets)))
    assert res[0][2] == res[1][2] and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0


def test_thirty_steps_reduce_the_loss():
    """The criterion of tests/test_step_gpu.py::test_overfits_one_fixed_batch on 30 MomentumSGD steps (lr 0.01, momentum 0.9, weight decay
    5e-4, which also decays gamma and beta) on one fixed batch: the total loss falls by at least half between its first and last five
    steps, every loss stays finite, the box-classification and mask losses both fall."""
    m, chain = _build(seed=11, head_norm='gn')
    opt = MomentumSGD(lr=0.01, momentum=0.9).setup(chain)
    opt.add_hook(WeightDecay(0.0005))
    b = _batch()
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss')
    hist = []
    for it in range(30):
        chain.proposal_target_creator.set_seed(100 + it)
        chain.anchor_target_creator.set_seed(200 + it)
        opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
        hist.append(torch.stack([chain.observation[k].detach() for k in names]))
    h = torch.stack(hist).cpu().numpy()
    assert np.isfinite(h).all(), np.argwhere(~np.isfinite(h))[:5]
    first, last = h[:5].mean(0), h[-5:].mean(0)
    print('first', first, 'last', last)
    assert last[5] <= 0.5 * first[5], (first, last)
    assert last[3] < first[3] and last[4] < first[4], (first, last)
    assert torch.isfinite(m.ps.params).all()
    gamma = m.ps.p('head/mask1/gn/gamma')
    assert not torch.equal(gamma[:m.head.channels], torch.ones_like(gamma[:m.head.channels]))      # the new parameters are trained


def test_keypoint_chain_runs_one_step():
    K = 17
    m = MaskRCNN(n_fg_class=1, n_keypoints=K, head_arch='fpn_keypoint', device=DEV, seed=11, _test_shrink=SHRINK, head_norm='gn')
    assert len(m.head.mask_gns) == 8 and all(g is not None for g in m.head.mask_gns)
    chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_keypoint_loss, binary_mask=False)
    b = make_batch(5, 2, 128, 160, G=3, n_fg_class=1, n_keypoints=K)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
    b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    chain(b['imgs'], b['bboxes'], b['labels'], b['keypoints'], 1.0).backward()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in chain.observation.values())
    assert torch.isfinite(m.ps.grads).all()
    for n in m.ps.names():
        if '/gn/' in n:
            assert float(m.ps.g(n).abs().max()) > 0, n


def test_graphed_step_with_group_norm_replays_the_eager_step():
    """optimizers.GraphedStep with GroupNorm in the heads: captured once (after 3 eager warm-up steps), one replay - the parameters of four
    eager steps, bit for bit."""
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build(head_norm='gn')
        b = _batch()
        step_harness.seed(chain)
        opt = MomentumSGD(lr=1e-2, momentum=0.9, high_priority_stream=False).setup(chain)
        opt.add_hook(WeightDecay(0.0005))
        batch = [b['imgs'], b['bboxes'], b['labels'], b['masks']]
        if graphed:
            g = GraphedStep(opt, chain, batch, 1.0, warmup=3)
            g(*batch)
        else:
            for _ in range(4):
                opt.update(chain, *batch, 1.0)
        torch.cuda.synchronize()
        res.append((m.ps.params.clone(), float(chain.observation['loss'])))
    assert res[0][1] == res[1][1]
    assert torch.equal(res[0][0], res[1][0])


# ---- inference ----------------------------------------------------------------------------------------------------------------------------
def test_predict_in_evaluation_mode_and_npz_round_trip(tmp_path):
    from chainer_maskrcnn.utils.chainer_npz import load_npz, save_npz
    m = _predict_model(5)
    g = torch.Generator().manual_seed(0)
    for n in m.ps.names():
        if '/gn/' in n:
            m.ps.p(n)[:m.head.channels] += (torch.randn(m.head.channels, generator=g) * 0.2).to(DEV)
    rs = np.random.RandomState(0)
    a, b = (torch.from_numpy((rs.rand(3, h, w) * 255).astype(np.float32)) for h, w in ((120, 150), (100, 100)))
    alone = m.predict([a])
    alone_boxes = m.last_bboxes
    assert m.train is True and core.TRAIN is True
    assert alone[1][0].shape[0] > 0
    with m._inference_mode():                       # evaluation mode keeps no statistics and no context
        y, ctx = m.head.gn1.fwd(torch.randn((3, 7, 7, m.head.conv1.cout_p), device=DEV), relu=True)
        assert ctx is None and y.shape == (3, 7, 7, m.head.conv1.cout_p)
    both = m.predict([b, a])                        # per-RoI statistics: no coupling across the images of a batch
    for k in range(3):
        assert torch.equal(alone[k][0], both[k][1])
    assert torch.equal(alone_boxes[0], m.last_bboxes[1])
    path = str(tmp_path / 'gn.npz')
    save_npz(path, m)
    fresh = _predict_model(6)
    assert not torch.equal(fresh.ps.params, m.ps.params)
    load_npz(path, fresh, strict=True)
    again = fresh.predict([a])
    for k in range(3):
        assert torch.equal(alone[k][0], again[k][0])
    assert torch.equal(alone_boxes[0], fresh.last_bboxes[0])
