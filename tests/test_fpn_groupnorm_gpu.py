"""GPU tests of GroupNorm in the FPN (csrc/groupnorm_map.hip, nn/core.py MapGroupNorm, FeaturePyramidNetwork(fpn_norm='gn'); DESIGN.md
section 3.23): the split-reduction kernels against the float64 reference of tests/fpn_groupnorm_reference.py, their bitwise properties,
the layer's dispatch, the top-down pyramid against float64 autograd on the CPU, the whole training step, inference, and the untouched
defaults."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'chainer-maskrcnn_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from chainer_maskrcnn.model.extractor.feature_pyramid_network import FeaturePyramidNetwork  # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_keypoint_loss  # noqa: E402
from chainer_maskrcnn.nn import core  # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay  # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch  # noqa: E402
import fpn_groupnorm_reference as fgr  # noqa: E402
from tests import step_harness  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
D = torch.float64
FWD_BAR, BWD_BAR = 1e-5, 2e-5          # the bars of tests/test_groupnorm_gpu.py


def _rel(got, ref):
    """The metric of tests/test_groupnorm_gpu.py."""
    got = got.double().cpu() if torch.is_tensor(got) else torch.as_tensor(got, dtype=D)
    ref = torch.as_tensor(ref, dtype=D)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _ppc(Cp):
    """pixels_per_chunk of a map small enough for one chunk: the chunk size the library was built with for this Cp."""
    return ops.group_norm_map_plan(1, 1, 1, Cp, Cp, Cp // 4)[0]


def _cases():
    p = _ppc(32)
    return [(1, 1, p, 32, 32, 8),                   # one chunk
            (2, 1, p + 1, 32, 32, 8),               # the second chunk holds one pixel
            (3, 1, 3 * p - 1, 32, 32, 8),           # three chunks
            (2, 37, 53, 48, 64, 12),                # padded channels, odd sizes
            (2, 40, 40, 128, 128, 2),               # cpg 64
            (2, 64, 64, 256, 256, 32),              # production channels
            (1, 256, 256, 256, 256, 32)]            # the P2 grid of one image


N_CASES = 7


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


def test_cases_reach_one_two_and_more_chunks():
    cases = _cases()
    assert len(cases) == N_CASES
    chunks = [ops.group_norm_map_plan(*c)[1] for c in cases]
    assert chunks[:3] == [1, 2, 3] and all(k >= 3 for k in chunks[3:]), chunks
    assert ops.group_norm_map_plan(*cases[1])[0] == _ppc(32)
    assert 1 * chunks[6] >= 256                              # the P2 grid of one image: a workgroup per CU and image
    assert all(ops.group_norm_plan(*c)[0] == 1 for c in cases[1:])   # above the register path's cap


def _run(case, x, gy, gamma, beta):
    R, H, W, C, Cp, G = case
    xd, gyd, gd, bd = _dev(x, gy, gamma, beta)
    y, mean, rstd = ops.group_norm_map_fwd(xd, gd, bd, C, G)
    gx, gg, gb = ops.group_norm_map_bwd(gyd, xd, gd, mean, rstd, C, G, gg=torch.full((Cp,), 7.0, device=DEV), gb=torch.full((Cp,), -7.0, device=DEV))
    return {'y': y, 'mean': mean, 'rstd': rstd, 'gx': gx, 'ggamma': gg, 'gbeta': gb}


def _errors(case, x, gy, gamma, beta, got):
    """{quantity: (device error, float32 floor)} against the float64 reference, in the _rel metric; the floor is the same computation
    carried out in float32 against the same float64 result."""
    R, H, W, C, Cp, G = case
    r64 = fgr.all_six(x.numpy(), gy.numpy(), gamma.numpy(), beta.numpy(), C, G, np.float64)
    r32 = fgr.all_six(x.numpy(), gy.numpy(), gamma.numpy(), beta.numpy(), C, G, np.float32)
    return {k: (_rel(got[k], r64[k]), _rel(r32[k], r64[k])) for k in r64}


@pytest.mark.parametrize('i', range(N_CASES))
def test_kernels_match_the_float64_reference(i):
    """Bar: the larger of the bars of tests/test_groupnorm_gpu.py (1e-5 forward, 2e-5 backward) and four times the float32 floor on the
    same data - the device's fixed summation tree is not NumPy's, and rstd enters every output."""
    case = _cases()[i]
    R, H, W, C, Cp, G = case
    x, gy, gamma, beta = _data(case)
    got = _run(case, x, gy, gamma, beta)
    errs = _errors(case, x, gy, gamma, beta, got)
    bad = []
    for k, (err, floor) in errs.items():
        bar = max(FWD_BAR if k in ('y', 'mean', 'rstd') else BWD_BAR, 4 * floor)
        print('%s %-6s err %.3e floor %.3e bar %.3e' % (case, k, err, floor, bar))
        if not err <= bar:
            bad.append((k, err, floor, bar))
    assert not bad, bad
    # exact zeros on the padding, whatever the padding of x and gy holds
    assert not got['y'][..., C:].any() and not got['gx'][..., C:].any() and not got['ggamma'][C:].any() and not got['gbeta'][C:].any()


@pytest.mark.parametrize('i', range(N_CASES))
def test_bitwise_properties(i):
    case = _cases()[i]
    R, H, W, C, Cp, G = case
    x, gy, gamma, beta = _data(case, seed=2)
    xd, gyd, gd, bd = _dev(x, gy, gamma, beta)
    y, mean, rstd = ops.group_norm_map_fwd(xd, gd, bd, C, G)
    y2, m2, r2 = ops.group_norm_map_fwd(xd, gd, bd, C, G, want_stats=False)
    assert m2 is None and r2 is None and torch.equal(y, y2)                     # the same y without the statistics
    y3, m3, r3 = ops.group_norm_map_fwd(xd, gd, bd, C, G)
    assert torch.equal(y, y3) and torch.equal(mean, m3) and torch.equal(rstd, r3)       # the same bits on every run
    a = ops.group_norm_map_bwd(gyd, xd, gd, mean, rstd, C, G)
    b = ops.group_norm_map_bwd(gyd, xd, gd, mean, rstd, C, G)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # the padding of x and gy decides nothing
    xz, gz = xd.clone(), gyd.clone()
    xz[..., C:] = 0
    gz[..., C:] = 0
    yz, mz, rz = ops.group_norm_map_fwd(xz, gd, bd, C, G)
    c = ops.group_norm_map_bwd(gz, xz, gd, mz, rz, C, G)
    assert torch.equal(y, yz) and torch.equal(mean, mz) and torch.equal(rstd, rz) and all(torch.equal(p, q) for p, q in zip(a, c))
    # accumulate_params adds to what is there
    g = torch.Generator().manual_seed(3)
    pre_g, pre_b = _dev(torch.randn(Cp, generator=g), torch.randn(Cp, generator=g))
    gg, gb = pre_g.clone(), pre_b.clone()
    gx, _, _ = ops.group_norm_map_bwd(gyd, xd, gd, mean, rstd, C, G, gg=gg, gb=gb, accumulate_params=True)
    assert torch.equal(gx, a[0])
    for got, pre, over in ((gg, pre_g, a[1]), (gb, pre_b, a[2])):
        want = pre + over
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float('inf'))) - want.abs()
        assert bool(((got - want).abs() <= ulp).all())
    assert torch.equal(gg[C:], pre_g[C:]) and torch.equal(gb[C:], pre_b[C:])


def test_empty_batch():
    x = torch.zeros((0, 40, 40, 64), device=DEV)
    gamma, beta = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    y, mean, rstd = ops.group_norm_map_fwd(x, gamma, beta, 64, 16)
    assert y.shape == (0, 40, 40, 64) and mean.shape == (0, 16) and rstd.shape == (0, 16)
    gx, gg, gb = ops.group_norm_map_bwd(x, x, gamma, mean, rstd, 64, 16)
    assert gx.shape == (0, 40, 40, 64) and not gg.any() and not gb.any()
    keep = torch.full((64,), 2.0, device=DEV)
    ops.group_norm_map_bwd(x, x, gamma, mean, rstd, 64, 16, gg=keep, gb=keep.clone(), accumulate_params=True)
    assert torch.equal(keep, torch.full((64,), 2.0, device=DEV))


def test_large_mean_keeps_its_digits():
    """x = randn + 100: the merged variance about the chunk means stays accurate where E[x^2] - E[x]^2 in float32 would not.  The bar for
    every quantity is 5e-4, that of tests/test_groupnorm_gpu.py::test_large_mean_keeps_its_digits."""
    case = (2, 64, 64, 256, 256, 32)
    x, gy, gamma, beta = _data(case, seed=1, offset=100.0, scale=1.0)
    got = _run(case, x, gy, gamma, beta)
    errs = _errors(case, x, gy, gamma, beta, got)
    print('large mean', {k: '%.3e (floor %.3e)' % v for k, v in errs.items()})
    assert all(e <= 5e-4 for e, _ in errs.values()), errs


# ---- the layer's dispatch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,path', [((2, 16, 16, 64, 64, 16), 0), ((2, 33, 31, 64, 64, 32), 1)], ids=['register', 'generic_cpg2'])
def test_layer_is_the_existing_kernels_where_the_map_path_does_not_apply(case, path):
    R, H, W, C, Cp, G = case
    assert ops.group_norm_plan(*case)[0] == path
    ps = core.ParamStore()
    gn = core.MapGroupNorm(ps, 'l/gn', C, G)
    ps.materialise(torch.device(DEV), 1)
    assert not gn.uses_map_path((R, H, W, Cp))
    x, gy, gamma, beta = _data(case, seed=4)
    xd, gyd, gd, bd = _dev(x, gy, gamma, beta)
    ps.p('l/gn/gamma').copy_(gd)
    ps.p('l/gn/beta').copy_(bd)
    assert core.TRAIN
    y, ctx = gn.fwd(xd)
    gx = gn.bwd(ctx, gyd)
    yr, mr, rr = ops.group_norm_fwd(xd, gd, bd, C, G)
    gxr, ggr, gbr = ops.group_norm_bwd(gyd, xd, gd, bd, mr, rr, C, G)
    assert ctx[0] is xd and torch.equal(ctx[1], mr) and torch.equal(ctx[2], rr)
    assert torch.equal(y, yr) and torch.equal(gx, gxr) and torch.equal(ps.g('l/gn/gamma'), ggr) and torch.equal(ps.g('l/gn/beta'), gbr)


def test_layer_takes_the_map_kernels_on_a_map_and_keeps_nothing_in_evaluation():
    case = (2, 37, 53, 64, 64, 16)
    R, H, W, C, Cp, G = case
    ps = core.ParamStore()
    gn = core.MapGroupNorm(ps, 'l/gn', C, G)
    ps.materialise(torch.device(DEV), 1)
    assert gn.uses_map_path((R, H, W, Cp))
    x, gy, gamma, beta = _data(case, seed=5)
    xd, gyd, gd, bd = _dev(x, gy, gamma, beta)
    ps.p('l/gn/gamma').copy_(gd)
    ps.p('l/gn/beta').copy_(bd)
    y, ctx = gn.fwd(xd)
    gx = gn.bwd(ctx, gyd)
    yr, mr, rr = ops.group_norm_map_fwd(xd, gd, bd, C, G)
    gxr, ggr, gbr = ops.group_norm_map_bwd(gyd, xd, gd, mr, rr, C, G)
    assert torch.equal(y, yr) and torch.equal(gx, gxr) and torch.equal(ps.g('l/gn/gamma'), ggr) and torch.equal(ps.g('l/gn/beta'), gbr)
    keep = core.TRAIN
    core.TRAIN = False
    try:
        y2, ctx2 = gn.fwd(xd)
    finally:
        core.TRAIN = keep
    assert ctx2 is None and torch.equal(y2, y)


# ---- the top-down pyramid against float64 autograd on the CPU ----------------------------------------------------------------------------
_check = step_harness.check


def test_pyramid_matches_float64_autograd():
    """The shrunk width (64 FPN channels, 16 groups of 4) on c2 .. c5 of odd sizes (the crop of upsample2x_add): P2 takes the map kernels,
    P5 the register-resident ones.  The stage outputs carry both signs, so the data gradients are compared where the input is positive
    (mask_gx: the ReLU backward of the stage below is applied where the gradient is written)."""
    G = 16
    fpn = FeaturePyramidNetwork(stages=(1, 1, 1, 1), width_div=4, fpn_norm='gn', gn_groups=G)
    ps = fpn.ps.materialise(torch.device(DEV), 3)
    fc = fpn.out_channels
    assert fc == 64
    g = torch.Generator().manual_seed(6)
    names = []
    for n in fgr.FPN_CONVS:
        names += ['extractor/%s/%s' % (n, k) for k in ('W', 'b', 'gn/gamma', 'gn/beta')]
        for k in ('b', 'gn/gamma', 'gn/beta'):          # off their 0 / 1 initial values
            ps.p('extractor/%s/%s' % (n, k)).add_((torch.randn(fc, generator=g) * 0.2).to(DEV))
    shapes = [(2, 37, 53, 64), (2, 19, 27, 128), (2, 10, 14, 256), (2, 5, 7, 512)]
    cs = [torch.randn(s, generator=g) for s in shapes]
    assert fpn.norms['extractor/conv_p2'].uses_map_path((2, 37, 53, fc)) and not fpn.norms['extractor/toplayer'].uses_map_path((2, 5, 7, fc))
    assert core.TRAIN
    pd = fpn.top_down(*_dev(*cs))
    assert [tuple(p.shape) for p in pd] == [(2, 37, 53, fc), (2, 19, 27, fc), (2, 10, 14, fc), (2, 5, 7, fc), (2, 3, 4, fc)]
    grads = [torch.randn(p.shape, generator=g) for p in pd]
    ps.grads.zero_()
    gcs = fpn.top_down_backward(_dev(*grads))
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    P = {n[len('extractor/'):]: ps.p(n).detach().cpu() for n in names}
    p64, gc64, gr64 = fgr.top_down(P, cs, grads, G, D)
    p32, gc32, gr32 = fgr.top_down(P, cs, grads, G, torch.float32)
    bad = []
    for i, lv in enumerate(('p2', 'p3', 'p4', 'p5', 'p6')):
        _check(lv, pd[i], p64[i], p32[i], bad)
    for i, lv in enumerate(('g_c2', 'g_c3', 'g_c4', 'g_c5')):
        m = (cs[i] > 0)
        _check(lv, gcs[i], gc64[i] * m, gc32[i] * m, bad)
    for n in names:
        _check(n, ps.g(n), gr64[n[len('extractor/'):]], gr32[n[len('extractor/'):]], bad)
    assert not bad, bad
    fpn.tape = None


# ---- the whole step -----------------------------------------------------------------------------------------------------------------------
SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)


_batch, _step = step_harness.batch, step_harness.step


def _build(**kw):
    kw.setdefault('gn_groups', 16)
    return step_harness.build(SHRINK, **kw)


def _gn_gradients_are_live(m):
    """Every GroupNorm parameter has a finite, non-zero gradient - conv_p6's exactly when its convolution has one: at these image sizes P6
    is 2 x 3 and a step in which the RPN samples none of its anchors sends no gradient into it."""
    for n in m.ps.names():
        if '/gn/' in n:
            g = m.ps.g(n)
            assert torch.isfinite(g).all(), n
            conv = n.split('/gn/')[0]
            assert (float(g.abs().max()) > 0) == ('/conv_p6' not in n or float(m.ps.g(conv + '/W').abs().max()) > 0), n


def test_step_with_fpn_norm_is_finite_and_bit_reproducible():
    m, chain = _build(fpn_norm='gn')
    b = _batch()
    assert m.extractor.norms['extractor/conv_p2'].uses_map_path((2, 32, 40, 64))       # the step runs the map kernels
    _step(chain, b)
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert all(np.isfinite(v) for v in obs.values()), obs
    g1 = m.ps.grads.clone()
    assert torch.isfinite(g1).all()
    assert sum('/gn/' in n for n in m.ps.names()) == 16
    _gn_gradients_are_live(m)
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)                      # no atomics in the map kernels either


@pytest.mark.parametrize('at', [2, 5])
def test_frozen_prefix_still_trains_the_fpn_norm(at):
    """freeze_at = 5 leaves no stage to take toplayer's data gradient; its GroupNorm backward still runs, because toplayer's filter gradient
    (and the GroupNorm's own parameters) need it.  The frozen ResNet parameters keep zero gradients, the FPN's GroupNorms do not."""
    m, chain = _build(fpn_norm='gn')
    m.freeze(bn=True, at=at)
    _step(chain, _batch())
    assert all(np.isfinite(float(v)) for v in chain.observation.values()) and torch.isfinite(m.ps.grads).all()
    _gn_gradients_are_live(m)
    assert float(m.ps.g('extractor/toplayer/W').abs().max()) > 0
    assert not any('/gn/' in n for n in m.ps.frozen)
    assert all(not m.ps.g(n).any() for n in m.ps.frozen)


def test_defaults_are_untouched():
    """fpn_norm=None and a model built without the argument: the same parameters, the same flat gradient buffer, bit for bit."""
    res = []
    for kw in ({}, {'fpn_norm': None}):
        m, chain = _build(**kw)
        _step(chain, _batch())
        res.append((m.ps.params.clone(), m.ps.grads.clone(), dict(m.ps.offsets)))
    assert res[0][2] == res[1][2] and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0 and not any('/gn/' in n for n in res[0][2])


def test_graphed_step_with_fpn_norm_replays_the_eager_step():
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build(fpn_norm='gn')
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


def test_thirty_steps_reduce_the_loss():
    """The setting of tests/test_groupnorm_gpu.py::test_thirty_steps_reduce_the_loss with fpn_norm='gn': the loss of the first and last
    five steps is printed; asserted is only that every loss is finite and the total is lower at the end."""
    m, chain = _build(seed=11, fpn_norm='gn')
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
    print('first five', h[:5, 5], 'last five', h[-5:, 5])
    assert last[5] < first[5], (first, last)
    assert torch.isfinite(m.ps.params).all()
    gamma = m.ps.p('extractor/conv_p2/gn/gamma')
    assert not torch.equal(gamma, torch.ones_like(gamma))      # the new parameters are trained


def test_images_of_a_batch_are_independent_in_evaluation_mode():
    """Statistics per sample: p2 .. p6 of image 0 keep their bits when image 1's pixels change (BatchNorm runs on its running statistics in
    evaluation mode, so GroupNorm is the only place two images could meet)."""
    m, _ = _build(fpn_norm='gn')
    g = torch.Generator().manual_seed(1)
    x = torch.zeros((2, 128, 160, 4))
    x[..., :3] = torch.rand((2, 128, 160, 3), generator=g)
    x2 = x.clone()
    x2[1, ..., :3] = torch.rand((128, 160, 3), generator=g)
    with m._inference_mode():
        a = m.extractor(x.to(DEV))
        b = m.extractor(x2.to(DEV))
    assert m.extractor.tape.get('p2/gn') is None            # evaluation keeps nothing
    for pa, pb in zip(a, b):
        assert torch.equal(pa[0], pb[0]) and not torch.equal(pa[1], pb[1])


def test_keypoint_chain_and_both_norms_run_one_step():
    K = 17
    m = MaskRCNN(n_fg_class=1, n_keypoints=K, head_arch='fpn_keypoint', device=DEV, seed=11, _test_shrink=SHRINK, fpn_norm='gn', gn_groups=16)
    chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_keypoint_loss, binary_mask=False)
    b = make_batch(5, 2, 128, 160, G=3, n_fg_class=1, n_keypoints=K)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
    b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    chain(b['imgs'], b['bboxes'], b['labels'], b['keypoints'], 1.0).backward()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in chain.observation.values())
    assert torch.isfinite(m.ps.grads).all()
    _gn_gradients_are_live(m)
    m, chain = _build(fpn_norm='gn', head_norm='gn')
    _step(chain, _batch())
    assert all(np.isfinite(float(v)) for v in chain.observation.values()) and torch.isfinite(m.ps.grads).all()
    assert sum('/gn/' in n for n in m.ps.names()) == 26
    _gn_gradients_are_live(m)


def test_predict_after_an_npz_round_trip(tmp_path):
    from chainer_maskrcnn.utils.chainer_npz import load_npz, save_npz

    def model(seed):
        m = MaskRCNN(n_fg_class=80, device=DEV, seed=seed, _test_shrink=SHRINK, min_size=160, max_size=260, fpn_norm='gn', gn_groups=16)
        m.use_preset('evaluate')
        m.score_thresh = 0.0125                     # random weights: ~uniform class probabilities (1/81 = 0.0123)
        return m
    m = model(5)
    g = torch.Generator().manual_seed(0)
    for n in m.ps.names():
        if '/gn/' in n:
            m.ps.p(n).add_((torch.randn(m.extractor.out_channels, generator=g) * 0.2).to(DEV))
    rs = np.random.RandomState(0)
    a = torch.from_numpy((rs.rand(3, 120, 150) * 255).astype(np.float32))
    alone = m.predict([a])
    boxes = m.last_bboxes
    assert m.train is True and core.TRAIN is True
    assert alone[1][0].shape[0] > 0
    path = str(tmp_path / 'gn.npz')
    save_npz(path, m)
    fresh = model(6)
    assert not torch.equal(fresh.ps.params, m.ps.params)
    load_npz(path, fresh, strict=True)
    again = fresh.predict([a])
    for k in range(3):
        assert torch.equal(alone[k][0], again[k][0])
    assert torch.equal(boxes[0], fresh.last_bboxes[0])
