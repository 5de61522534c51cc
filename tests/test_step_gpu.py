"""GPU parity test of the WHOLE training step: device losses and every parameter gradient against the CPU
oracle (oracle/model.py: float64 torch autograd + NumPy ROIAlign) on a width/depth-reduced network, with the
device's sampled targets fed to the oracle (the samplers are pinned in test_targets_gpu.py / test_rpn_gpu.py).
Tolerance: 1e-3 relative (BASELINE.json north_star); observed ~1e-5."""
import numpy as np
import pytest
import torch

from oracle.model import OracleStep, D

pytestmark = pytest.mark.gpu

from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss, calc_keypoint_loss  # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay  # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch  # noqa: E402
from tests import step_harness  # noqa: E402

DEV = 'cuda:0'
STAGES = (2, 1, 1, 1)
SHRINK = dict(stages=STAGES, width_div=2)


_batch, _grad_ok = step_harness.batch, step_harness.grad_ok


def _build(mask_rows, seed=7):
    return step_harness.build(SHRINK, seed, mask_rows=mask_rows)


@pytest.mark.parametrize('mask_rows', ['positives', 'all'])
def test_step_losses_and_gradients_match_oracle(mask_rows, grad_tol=1e-3):
    m, chain = _build(mask_rows)
    b = _batch()
    loss = chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
    loss.backward()
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert abs(float(loss.detach()) - sum(obs[k] for k in obs if k != 'loss')) < 1e-5
    # ---- oracle on the same weights and the device's targets
    ps = m.ps
    params = {n: ps.p(n).detach().cpu().to(D).requires_grad_(True) for n in ps.names()}
    t = {k: v.cpu().numpy() for k, v in chain.targets.items() if torch.is_tensor(v)}
    t['gt_rpn_loc'], t['gt_rpn_label'] = (x.cpu().numpy() for x in chain.rpn_targets)
    t['mask_rois_xy5'], t['mask_levels'], t['mask_label'] = (x.cpu().numpy() for x in chain.mask_inputs)
    assert (t['gt_roi_label'] > 0).sum() >= 4 and (t['gt_rpn_label'] == 1).sum() >= 2      # the case exercises every loss
    oracle = OracleStep(params, STAGES, m.head.n_class, m.head.LOC0)
    img4 = torch.cat([b['imgs'].cpu().permute(0, 2, 3, 1), torch.zeros((2, 128, 160, 1))], -1).to(D)
    out = oracle.losses(img4, t)
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss')
    for k in names:
        ok_ = float(out[k].detach())
        assert abs(obs[k] - ok_) <= 1e-4 * max(abs(ok_), 1e-3), (k, obs[k], ok_)
    sum(out[k] for k in names).backward()
    # float32 noise floor of this network: the same oracle step evaluated in float32 (tests/test_full_width_gpu.py has the
    # long version).  The bar is grad_tol, or 3 x that floor where the float32 oracle itself is further away - a ReLU /
    # max-pool decision on a value within rounding of a tie moves single tensors by ~1e-3 in ANY float32 evaluation.
    from oracle import model as om
    om.set_dtype(torch.float32)
    try:
        p32 = {n: ps.p(n).detach().cpu().requires_grad_(True) for n in ps.names()}
        out32 = OracleStep(p32, STAGES, m.head.n_class, m.head.LOC0).losses(img4.float(), t)
        sum(out32[k] for k in names).backward()
    finally:
        om.set_dtype(torch.float64)
    worst = 0.0
    gmax = max(float(params[n].grad.abs().max()) for n in ps.names() if params[n].grad is not None)
    for n in ps.names():
        want = params[n].grad
        want = torch.zeros_like(params[n]) if want is None else want
        w32 = p32[n].grad if p32[n].grad is not None else torch.zeros_like(p32[n])
        got = ps.g(n).cpu().to(D)
        # biases in front of a BatchNorm have an exactly-zero gradient: floor the scale at 1e-3 of the largest gradient
        scale = max(float(want.abs().max()), 1e-3 * gmax)
        err = float((got - want).abs().max()) / scale
        floor = float((w32.to(D) - want).abs().max()) / scale
        worst = max(worst, err)
        assert _grad_ok(got, want, err, floor, grad_tol), (n, err, floor)
    print('worst relative gradient error', worst)


def test_keypoint_step_matches_oracle():
    """BASELINE config 5 head (train_keypoints.py): 17 keypoints, 56x56 heat maps, softmax CE over positions."""
    K, NMC = 17, 2
    m = MaskRCNN(n_fg_class=1, n_keypoints=K, n_mask_convs=NMC, head_arch='fpn_keypoint', device=DEV, seed=11,
                 _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2))
    chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_keypoint_loss, binary_mask=False)
    b = make_batch(5, 2, 128, 160, G=3, n_fg_class=1, n_keypoints=K)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
    b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    loss = chain(b['imgs'], b['bboxes'], b['labels'], b['keypoints'], 1.0)
    loss.backward()
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert m.head.mask_size == 56 and chain.targets['gt_roi_mask'].shape[1] == K
    ps = m.ps
    params = {n: ps.p(n).detach().cpu().to(D).requires_grad_(True) for n in ps.names()}
    t = {k: v.cpu().numpy() for k, v in chain.targets.items() if torch.is_tensor(v)}
    t['gt_rpn_loc'], t['gt_rpn_label'] = (x.cpu().numpy() for x in chain.rpn_targets)
    t['mask_rois_xy5'], t['mask_levels'], t['mask_label'] = (x.cpu().numpy() for x in chain.mask_inputs)
    assert (t['gt_roi_mask'] >= 0).sum() > 10
    oracle = OracleStep(params, (1, 1, 1, 1), m.head.n_class, m.head.LOC0,
                        mask_conv_names=['mask_convs/%d' % i for i in range(NMC)], n_keypoints=K)
    img4 = torch.cat([b['imgs'].cpu().permute(0, 2, 3, 1), torch.zeros((2, 128, 160, 1))], -1).to(D)
    out = oracle.losses(img4, t)
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss')
    for k in names:
        assert abs(obs[k] - float(out[k].detach())) <= 1e-4 * max(abs(float(out[k].detach())), 1e-3), (k, obs[k], float(out[k].detach()))
    sum(out[k] for k in names).backward()
    # fp32 noise floor of this (tiny-batch BatchNorm) network: the same oracle evaluated in float32
    from oracle import model as om
    om.set_dtype(torch.float32)
    try:
        p32 = {n: ps.p(n).detach().cpu().requires_grad_(True) for n in ps.names()}
        o32 = OracleStep(p32, (1, 1, 1, 1), m.head.n_class, m.head.LOC0,
                         mask_conv_names=['mask_convs/%d' % i for i in range(NMC)], n_keypoints=K)
        out32 = o32.losses(img4.float(), t)
        sum(out32[k] for k in names).backward()
    finally:
        om.set_dtype(torch.float64)
    gmax = max(float(params[n].grad.abs().max()) for n in ps.names() if params[n].grad is not None)
    for n in ps.names():
        want = params[n].grad if params[n].grad is not None else torch.zeros_like(params[n])
        w32 = p32[n].grad if p32[n].grad is not None else torch.zeros_like(p32[n])
        scale = max(float(want.abs().max()), 1e-3 * gmax)
        err = float((ps.g(n).cpu().to(D) - want).abs().max()) / scale
        floor = float((w32.to(D) - want).abs().max()) / scale
        assert _grad_ok(ps.g(n).cpu().to(D), want, err, floor, 1e-3), (n, err, floor)


def test_step_is_bit_reproducible_and_sgd_updates():
    m, chain = _build('positives')
    b = _batch()
    step_harness.seed(chain)
    chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
    g1 = m.ps.grads.clone()
    l1 = float(chain.observation['loss'])
    step_harness.seed(chain)
    chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
    assert float(chain.observation['loss']) == l1
    assert torch.equal(g1, m.ps.grads)                      # no atomics anywhere on the path
    opt = MomentumSGD(lr=1e-2, momentum=0.9).setup(chain)
    opt.add_hook(WeightDecay(0.0005))
    p0 = m.ps.params.clone()
    first = None
    for _ in range(12):
        opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
        first = first if first is not None else float(chain.observation['loss'])
    assert not torch.equal(p0, m.ps.params)
    assert float(chain.observation['loss']) < first        # it trains
    assert torch.isfinite(m.ps.params).all()


def test_sectioned_update_gives_the_same_bits_as_the_single_pass():
    """MomentumSGD.sectioned_update (round 5): the SGD step of a slice of the flat parameter buffer is enqueued as soon as the backward pass
    has left it, on its own stream, instead of one pass over everything behind the last gradient.  Same parameters, momentum and
    losses bit for bit after three steps; the sections tile the buffer from its end, once per step, and most of them are issued
    while the backward pass is still being enqueued."""
    b = _batch()
    outs = []
    for sectioned in (False, True):
        m, chain = _build('positives')
        step_harness.seed(chain)
        opt = MomentumSGD(lr=1e-2, momentum=0.9, sectioned_update=sectioned).setup(chain)
        opt.LOCAL_BUCKET_BYTES = 256 << 10
        opt.add_hook(WeightDecay(0.0005))
        calls = []
        inner = opt._sgd_section

        def spy(start, end, inner=inner, chain=chain, calls=calls):
            calls.append((start, end, chain.pending is not None))
            inner(start, end)
        opt._sgd_section = spy
        losses = []
        for _ in range(3):
            opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
            losses.append(float(chain.observation['loss']))
        torch.cuda.synchronize()
        assert chain.grad_ready_hook is None            # the optimizer listens only during its own update
        outs.append((m.ps.params.clone(), m.ps.momentum.clone(), losses, calls, m.ps.params.numel()))
    (p0, v0, l0, c0, n), (p1, v1, l1, c1, _) = outs
    assert not c0 and len(c1) % 3 == 0 and len(c1) >= 3 * 8
    step = c1[:len(c1) // 3]
    assert step[0][1] == n and step[-1][0] == 0 and all(step[i][0] == step[i + 1][1] for i in range(len(step) - 1))
    assert all(s0 % 64 == 0 for s0, _, _ in step)
    assert sum(1 for _, _, inside in step if inside) >= len(step) // 2
    assert l0 == l1
    assert torch.equal(p0, p1) and torch.equal(v0, v1)


def test_reference_api_surface():
    m, chain = _build('positives')
    with pytest.raises(ValueError):
        MaskRCNN(n_fg_class=None)
    with pytest.raises(ValueError):
        MaskRCNN(n_fg_class=3, backbone='vgg')
    with pytest.raises(ValueError):
        MaskRCNN(n_fg_class=3, head_arch='nope')
    strict = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, strict_batch1=True)
    b = _batch()
    with pytest.raises(ValueError):
        strict(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
    assert m.n_class == 81 and m.head.mask_size == 28
    assert m.extractor.feat_strides == [4, 8, 16, 32, 64] and m.extractor.anchor_sizes == [32, 64, 128, 256, 512]
    m.use_preset('evaluate')
    assert (m.nms_thresh, m.score_thresh) == (0.3, 0.05)
    # reference forward signature (maskrcnn.py:135-155), train mode
    m.train = True
    roi_cls_locs, roi_scores, rois, roi_indices, mask = m(b['imgs'][:1], 1.0)
    R = rois.shape[0]
    assert roi_cls_locs.shape == (R, 4) and roi_scores.shape == (R, 81) and mask.shape == (R, 80, 28, 28)
    assert roi_indices.shape == (R,) and R <= 2000


@pytest.mark.parametrize('name,tile,pass_tiles,grad_tol', [pytest.param('f2', 2, (0, 0, 0), 1e-3, marks=pytest.mark.gpu_long), ('shipped', 0, (2, 0, 0), 1e-3),
                                                           pytest.param('fast_f4', 4, (0, 0, 0), 3e-3, marks=pytest.mark.gpu_long)])
def test_step_matches_oracle_with_winograd_everywhere(name, tile, pass_tiles, grad_tol):
    """The same whole-step parity check with the Winograd thresholds lowered so that every 3x3 / stride-1 layer of the
    small test network (ResNet conv2's, FPN, RPN, box and mask heads) takes the Winograd kernels in all three passes:
    F(2x2,3x3) everywhere; the shipped per-pass choice (forward F(2x2), backward passes whichever of F(2x2) / F(4x4)
    needs fewer multiplications); F(4x4) everywhere (the opt-in fast mode: losses as tight, gradients at 3e-3 - forward
    F(4x4) rounding amplified by the losses' curvature, see tests/test_full_width_gpu.py)."""
    from chainer_maskrcnn import _hip
    _hip.check(_hip.lib().mrcnn_conv2d_set_winograd_thresholds(32, 64, tile))
    _hip.check(_hip.lib().mrcnn_conv2d_set_winograd_pass_tiles(*pass_tiles))
    try:
        test_step_losses_and_gradients_match_oracle('all', grad_tol=grad_tol)
    finally:
        _hip.check(_hip.lib().mrcnn_conv2d_set_winograd_thresholds(256, 2048, 0))
        _hip.check(_hip.lib().mrcnn_conv2d_set_winograd_pass_tiles(2, 0, 0))


def _user_mask_loss(roi_cls_mask, gt_roi_mask, xp, gt_roi_label):
    """The body of the reference's train.py:50-58, verbatim up to the module that provides sigmoid_cross_entropy
    (chainer.functions there, chainer_maskrcnn.functions here).  No ``fused_kind`` tag: the chain must CALL it."""
    from chainer_maskrcnn import functions as F
    roi_mask = roi_cls_mask[xp.arange(
        roi_cls_mask.shape[0]), gt_roi_label - 1]
    return F.sigmoid_cross_entropy(roi_mask[:gt_roi_mask.shape[0]],
                                   gt_roi_mask)


def _user_keypoint_loss(roi_cls_mask, gt_roi_mask, xp, gt_roi_label, num_keypoints=17):
    """train_keypoints.py:21-27 verbatim (same substitution)."""
    from chainer_maskrcnn import functions as F
    num_positives = gt_roi_mask.shape[0]
    roi_mask = roi_cls_mask[:num_positives].reshape(
        (num_positives * num_keypoints, -1))
    gt_roi_mask = gt_roi_mask.reshape((-1,))
    return F.softmax_cross_entropy(roi_mask, gt_roi_mask)


@pytest.mark.parametrize('kind', ['mask', 'keypoint'])
def test_user_supplied_mask_loss_fun_matches_fused_kernel(kind):
    """VERDICT r1 item 6 / ADVICE: FPNMaskRCNNTrainChain accepts an arbitrary callable like the reference
    (train.py:98, fpn_maskrcnn_train_chain.py:103-104).  A user-written copy of the reference's loss function, run through
    the generic path (HIP-backed select / sigmoid CE / softmax CE under torch autograd), must give the fused kernel's loss
    and parameter gradients; the exported calc_mask_loss / calc_keypoint_loss are real callables too."""
    if kind == 'mask':
        mk = lambda f: FPNMaskRCNNTrainChain(MaskRCNN(n_fg_class=80, device=DEV, seed=7, _test_shrink=dict(stages=STAGES, width_div=2)),
                                             mask_loss_fun=f, mask_rows='all')
        b = _batch()
        args = (b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
        fused_fun, user_fun = calc_mask_loss, _user_mask_loss
    else:
        mk = lambda f: FPNMaskRCNNTrainChain(MaskRCNN(n_fg_class=1, n_keypoints=17, n_mask_convs=2, head_arch='fpn_keypoint', device=DEV,
                                                      seed=11, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2)),
                                             mask_loss_fun=f, binary_mask=False, mask_rows='all')
        b = make_batch(5, 2, 128, 160, G=3, n_fg_class=1, n_keypoints=17)
        b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
        b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
        args = (b['imgs'], b['bboxes'], b['labels'], b['keypoints'], 1.0)
        fused_fun, user_fun = calc_keypoint_loss, _user_keypoint_loss
    res = {}
    for name, f in (('fused', fused_fun), ('user', user_fun)):
        chain = mk(f)
        assert chain.mask_loss_kind == ('generic' if name == 'user' else chain.mask_loss_kind)
        step_harness.seed(chain)
        loss = chain(*args)
        loss.backward()
        res[name] = (float(chain.observation['mask_loss']), float(loss.detach()), chain.faster_rcnn.ps.grads.clone())
    assert abs(res['user'][0] - res['fused'][0]) <= 1e-6 * max(abs(res['fused'][0]), 1.0), (res['user'][0], res['fused'][0])
    assert abs(res['user'][1] - res['fused'][1]) <= 1e-6 * max(abs(res['fused'][1]), 1.0)
    gf, gu = res['fused'][2], res['user'][2]
    # same arithmetic per row; the generic path orders the mask rows positives-first without padding rows, so the
    # filter-gradient sums run in another order: compare at float32 summation noise
    assert float((gf - gu).abs().max()) <= 2e-5 * float(gf.abs().max())
    # loss scaling: (loss * k).backward() scales every gradient by k (the upstream gradient is honoured)
    chain = mk(fused_fun)
    step_harness.seed(chain)
    (chain(*args) * 4.0).backward()
    assert float((chain.faster_rcnn.ps.grads - 4.0 * gf).abs().max()) <= 1e-5 * 4.0 * float(gf.abs().max())


def test_exported_loss_functions_are_callable():
    """calc_mask_loss / calc_keypoint_loss called directly (outside the chain) on device tensors."""
    from chainer_maskrcnn.functions.loss import MaskLogits, XP
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(0)
    R, C, S, n_pos = 12, 5, 6, 4
    x = torch.from_numpy(rs.standard_normal((R, C, S, S)).astype(np.float32)).to(DEV).requires_grad_(True)
    gt = torch.from_numpy(rs.randint(-1, 2, (n_pos, S, S)).astype(np.int32)).to(DEV)
    lab = torch.from_numpy(np.array([1, 3, 5, 2] + [0] * (R - n_pos), np.int32)).to(DEV)
    loss = calc_mask_loss(x.as_subclass(MaskLogits), gt, XP(x.device), lab)
    loss.backward()
    xn, gn, ln = x.detach().cpu().numpy().astype(np.float64), gt.cpu().numpy(), lab.cpu().numpy()
    sel = xn[np.arange(n_pos), ln[:n_pos] - 1]
    valid = gn != -1
    want = (np.maximum(sel, 0) - sel * gn + np.log1p(np.exp(-np.abs(sel))))[valid].sum() / valid.sum()
    assert abs(float(loss.detach()) - want) < 1e-5
    gwant = np.zeros_like(xn)
    gwant[np.arange(n_pos), ln[:n_pos] - 1] = np.where(valid, (1 / (1 + np.exp(-sel)) - gn) / valid.sum(), 0)
    np.testing.assert_allclose(x.grad.cpu().numpy(), gwant, atol=1e-6)
    K = 3
    xk = torch.from_numpy(rs.standard_normal((R, K, S, S)).astype(np.float32)).to(DEV).requires_grad_(True)
    gk = torch.from_numpy(rs.randint(-1, S * S, (n_pos, K)).astype(np.int32)).to(DEV)
    lk = calc_keypoint_loss(xk.as_subclass(MaskLogits), gk, XP(xk.device), lab, num_keypoints=K)
    lk.backward()
    xr = xk.detach().cpu().double().numpy()[:n_pos].reshape(n_pos * K, -1)
    tr = gk.cpu().numpy().reshape(-1)
    lse = np.log(np.exp(xr - xr.max(1, keepdims=True)).sum(1)) + xr.max(1)
    v = tr != -1
    assert abs(float(lk) - (lse[v] - xr[v, tr[v]]).sum() / v.sum()) < 1e-5
    assert float(xk.grad[n_pos:].abs().max()) == 0.0


@pytest.mark.parametrize('H,W', [(100, 132), (97, 151), (130, 66)])
def test_odd_image_sizes_whole_step_matches_oracle(H, W):
    """Sizes that are not multiples of 64: the stride-2 layers round up, max_pooling_2d covers the last odd row, and the
    top-down pathway crops F.unpooling_2d's output to the lateral's size (feature_pyramid_network.py:57-66).  Whole step
    (five losses, every parameter gradient) against the oracle on such tensors, batch 2."""
    m, chain = _build('positives')
    b = make_batch(5, 2, H, W, G=3)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [H, W])
    b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    chain.keep_outputs = True
    loss = chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
    loss.backward()
    obs = {k: float(v) for k, v in chain.observation.items()}
    ps = m.ps
    params = {n: ps.p(n).detach().cpu().to(D).requires_grad_(True) for n in ps.names()}
    t = {k: v.cpu().numpy() for k, v in chain.targets.items() if torch.is_tensor(v)}
    t['gt_rpn_loc'], t['gt_rpn_label'] = (x.cpu().numpy() for x in chain.rpn_targets)
    t['mask_rois_xy5'], t['mask_levels'], t['mask_label'] = (x.cpu().numpy() for x in chain.mask_inputs)
    oracle = OracleStep(params, STAGES, m.head.n_class, m.head.LOC0)
    img4 = torch.cat([b['imgs'].cpu().permute(0, 2, 3, 1), torch.zeros((2, H, W, 1))], -1).to(D)
    out = oracle.losses(img4, t)
    shapes = [tuple(f.shape[1:3]) for f in out['feats']]
    half = lambda n: (n - 1) // 2 + 1
    pool = lambda n: -(-(n - 2) // 2) + 1
    want = [(pool(half(H)), pool(half(W)))]
    for _ in range(4):
        want.append((half(want[-1][0]), half(want[-1][1])))
    assert shapes == want and [tuple(f.shape[1:3]) for f in chain.outputs['features']] == want
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss')
    for k in names:
        ok_ = float(out[k].detach())
        assert abs(obs[k] - ok_) <= 1e-4 * max(abs(ok_), 1e-3), (k, obs[k], ok_)
    sum(out[k] for k in names).backward()
    from oracle import model as om
    om.set_dtype(torch.float32)          # the float32 oracle = this network's own noise floor (see the first test of this file)
    try:
        p32 = {n: ps.p(n).detach().cpu().requires_grad_(True) for n in ps.names()}
        out32 = OracleStep(p32, STAGES, m.head.n_class, m.head.LOC0).losses(img4.float(), t)
        sum(out32[k] for k in names).backward()
    finally:
        om.set_dtype(torch.float64)
    gmax = max(float(params[n].grad.abs().max()) for n in ps.names() if params[n].grad is not None)
    for n in ps.names():
        want_g = params[n].grad if params[n].grad is not None else torch.zeros_like(params[n])
        w32 = p32[n].grad if p32[n].grad is not None else torch.zeros_like(p32[n])
        got = ps.g(n).cpu().to(D)
        scale = max(float(want_g.abs().max()), 1e-3 * gmax)
        err = float((got - want_g).abs().max()) / scale
        floor = float((w32.to(D) - want_g).abs().max()) / scale
        assert _grad_ok(got, want_g, err, floor, 1e-3), (n, err, floor)


def test_ragged_batch_padding_rows_are_ignored():
    """dataset/loader.py pads ragged batches with zero boxes / label -1 and train.py passes no counts.
    The chain must count the valid rows itself (#label >= 0, on the device); a zero box treated as a gt would make every
    inside anchor positive (ChainerCV's gt-argmax rule)."""
    from chainer_maskrcnn._hip import ops
    m, chain = _build('positives')
    b = _batch(G=3)
    bb, lab, mk = b['bboxes'].clone(), b['labels'].clone(), b['masks'].clone()
    bb[1, 1:] = 0
    lab[1, 1:] = -1
    mk[1, 1:] = 0
    chain.use_aux_stream = False
    chain(b['imgs'], bb, lab, mk, 1.0)                       # only to learn the key shapes
    A = chain.rpn_out['anchors'].shape[0]
    roi_cap = chain.rpn_out['rois'].shape[0] // 2
    pk = ops.random_keys((2, roi_cap + 3), 77, DEV)
    ak = ops.random_keys((2, A), 78, DEV)
    chain.sampler_keys = (pk, ak)
    snap = lambda: ({k: v.clone() for k, v in chain.targets.items() if torch.is_tensor(v)}, [x.clone() for x in chain.rpn_targets],
                    float(chain.observation['loss']))
    chain(b['imgs'], bb, lab, mk, 1.0)                       # counts derived from the labels
    t_auto, r_auto, l_auto = snap()
    chain(b['imgs'], bb, lab, mk, 1.0, n_gt=torch.tensor([3, 1], dtype=torch.int32, device=DEV))
    t_exp, r_exp, l_exp = snap()
    assert l_auto == l_exp
    for k in t_auto:
        assert torch.equal(t_auto[k], t_exp[k]), k
    assert torch.equal(r_auto[1], r_exp[1]) and torch.equal(r_auto[0], r_exp[0])
    # image 1 alone, un-padded (one gt), gives the same anchor targets as its padded row of the batch
    loc1, lab1 = chain.anchor_target_creator(bb[1:2, :1].contiguous(), chain.rpn_out['anchors'], (128, 160), keys=ak[1:2].contiguous())
    assert torch.equal(lab1[0], r_auto[1][1]) and torch.equal(loc1[0], r_auto[0][1])
    n_pos_anchor = int((r_auto[1][1] == 1).sum())
    assert 1 <= n_pos_anchor <= 128
    # and no padded gt row was sampled as a RoI: every sampled source index of image 1 is a proposal or gt row 0
    src = t_auto['sample_src'][256:256 + int(t_auto['n_sampled'][1])]
    n_roi1 = int(chain.rpn_out['n_rois'][1])
    assert int(src.max()) <= n_roi1


def test_image_without_objects_is_a_background_only_example():
    """An image whose every gt row is padding (label -1): the reference's step raises there (ChainerCV's AnchorTargetCreator
    takes an argmax over an empty axis); here it is a well-defined background-only example - all anchors of the image that
    are sampled are negatives, all its sampled RoIs are background with no mask target - and the step stays finite."""
    m, chain = _build('positives')
    b = _batch(G=3)
    bb, lab, mk = b['bboxes'].clone(), b['labels'].clone(), b['masks'].clone()
    bb[1] = 0
    lab[1] = -1
    mk[1] = 0
    loss = chain(b['imgs'], bb, lab, mk, 1.0)
    loss.backward()
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert all(np.isfinite(v) for v in obs.values()), obs
    assert bool(torch.isfinite(m.ps.grads).all())
    gt_rpn_loc, gt_rpn_label = chain.rpn_targets
    assert int((gt_rpn_label[1] == 1).sum()) == 0 and int((gt_rpn_label[1] == 0).sum()) == 256
    assert int((gt_rpn_label[0] == 1).sum()) >= 1
    t = chain.targets
    assert int(t['n_pos'][1]) == 0 and int(t['n_sampled'][1]) >= 1
    lab1 = t['gt_roi_label'][256:256 + int(t['n_sampled'][1])]
    assert int(lab1.abs().max()) == 0
    assert float(t['gt_roi_loc'][256:512].abs().max()) == 0.0 or int(t['n_pos'][1]) == 0
    # both images without objects: every loss term that needs a positive is exactly zero
    bb[0] = 0
    lab[0] = -1
    mk[0] = 0
    loss = chain(b['imgs'], bb, lab, mk, 1.0)
    loss.backward()
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert all(np.isfinite(v) for v in obs.values()), obs
    assert obs['rpn_loc_loss'] == 0.0 and obs['roi_loc_loss'] == 0.0 and obs['mask_loss'] == 0.0
    assert obs['rpn_cls_loss'] > 0.0 and obs['roi_cls_loss'] > 0.0
    assert bool(torch.isfinite(m.ps.grads).all())


def test_padded_batch_uses_each_images_own_size_and_scale():
    """dataset/loader.py hands over 'scales' (N,) and 'sizes' (N,2): the chain clips proposals to / tests anchors against
    each image's own size and filters with min_size * its own scale (the reference step is batch 1 per process:
    fpn_maskrcnn_train_chain.py:60-70).  Image 0 of the batch must see exactly what a scalar call with its size sees."""
    m, chain = _build('positives')
    b = _batch(G=3)
    chain.use_aux_stream = False
    chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
    A = chain.rpn_out['anchors'].shape[0]
    from chainer_maskrcnn._hip import ops
    ak = ops.random_keys((2, A), 78, DEV)
    sizes = np.array([[128, 160], [100, 131]], np.float32)
    scales = np.array([1.0, 1.6], np.float32)
    bb = b['bboxes'].clone()
    bb[1] = torch.minimum(bb[1], torch.tensor([100., 131., 100., 131.], device=DEV))
    chain.sampler_keys = (None, ak)
    chain(b['imgs'], bb, b['labels'], b['masks'], scales, img_sizes=sizes)
    rois = chain.rpn_out['rois'].reshape(2, -1, 4)
    n1 = int(chain.rpn_out['n_rois'][1])
    assert float(rois[1, :n1, 2].max()) <= 100 and float(rois[1, :n1, 3].max()) <= 131
    hw = rois[1, :n1, 2:] - rois[1, :n1, :2]
    assert float(hw.min()) >= chain.faster_rcnn.rpn.proposal_layer.min_size * 1.6
    lab_batch = chain.rpn_targets[1].clone()
    rois0 = rois[0].clone()
    # image 1's anchor labels = a batch-1 call with its own size; image 0 is untouched by image 1's smaller size
    loc1, lab1 = chain.anchor_target_creator(bb[1:2].contiguous(), chain.rpn_out['anchors'], (100, 131), keys=ak[1:2].contiguous())
    assert torch.equal(lab1[0], lab_batch[1])
    chain(b['imgs'], bb, b['labels'], b['masks'], 1.0)
    assert torch.equal(chain.rpn_out['rois'].reshape(2, -1, 4)[0], rois0)
    assert not torch.equal(chain.rpn_targets[1][1], lab_batch[1])
    chain.sampler_keys = None


@pytest.mark.parametrize('arith', ['f32', 'bf16x6_behind_backbone'])
def test_overfits_one_fixed_batch(arith):
    """Does it learn: 150 MomentumSGD steps (lr 0.01, momentum 0.9, weight decay 5e-4 - train.py's
    optimiser at a learning rate that fits the reduced network) on ONE fixed batch with fixed sampler seeds: the total
    loss falls by at least half, every one of the five losses stays finite at every step, and the box-classification and
    mask losses - the two that depend on the whole chain of proposals -> targets -> heads - both fall.  In the all-float32
    arithmetic and in the shipped one (train.py's default: the float32-accurate bf16x6 emulation everywhere but the backbone's forward pass)."""
    m, chain = _build('all', seed=11)
    chain.gemm_arithmetic = arith
    opt = MomentumSGD(lr=0.01, momentum=0.9).setup(chain)
    opt.add_hook(WeightDecay(0.0005))
    b = _batch()
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss')
    hist = []
    for it in range(150):
        chain.proposal_target_creator.set_seed(100 + it)
        chain.anchor_target_creator.set_seed(200 + it)
        opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
        hist.append(torch.stack([chain.observation[k].detach() for k in names]))
    h = torch.stack(hist).cpu().numpy()                  # one device->host copy at the end
    assert np.isfinite(h).all(), np.argwhere(~np.isfinite(h))[:5]
    first, last = h[:5].mean(0), h[-5:].mean(0)
    assert last[5] <= 0.5 * first[5], (first, last)
    assert last[3] < first[3] and last[4] < first[4], (first, last)
    assert torch.isfinite(m.ps.params).all()
    from chainer_maskrcnn import _hip
    _hip.check(_hip.lib().mrcnn_conv2d_set_split_operands(0, 0, 0))


def test_relu_mask_in_the_producer_gives_the_same_bits():
    """(r3) The ReLU backward of a bottleneck's output is applied by the kernels that write that output's gradient (data-gradient
    epilogues of the next block's conv1 / conv4, of toplayer and the laterals, the lattice scatter of the strided blocks) instead of by
    the block's bn3 backward (one stream less in each of its two kernels, no separate shortcut gradient): the same masks on the same
    sums, so every parameter gradient is bit-identical to the round-2 data flow (MASK_IN_PRODUCER = False)."""
    import chainer_maskrcnn.model.extractor.feature_pyramid_network as F
    grads = {}
    try:
        for flag in (True, False):
            F.MASK_IN_PRODUCER = flag
            m, chain = _build('all')
            b = _batch()
            chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
            grads[flag] = {n: m.ps.g(n).clone() for n in m.ps.names() if m.ps.g(n) is not None}
    finally:
        F.MASK_IN_PRODUCER = True
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) > 50
    for n in grads[True]:
        assert torch.equal(grads[True][n], grads[False][n]), n


def test_early_rpn_backward_gives_the_same_gradients():
    """MomentumSGD.update() tells the chain that a backward pass follows; the chain then runs the RPN's own backward pass on the aux
    stream right after the RPN losses, beside the proposal chain of the forward pass, and adds its per-level feature gradients where
    rpn.backward() used to run.  Same losses bit for bit; gradients: the RPN's own parameters bit for bit (same kernels, same order),
    everything below the pyramid to float32 rounding of ONE addition per feature element (old + (s0 + s1) instead of (old + s0) + s1
    on the levels whose data gradient is a split-K sum)."""
    res = {}
    for early in (False, True):
        m, chain = _build('all')
        b = _batch()
        step_harness.seed(chain)
        FPNMaskRCNNTrainChain.EARLY_RPN_BACKWARD = early
        try:
            opt = MomentumSGD(lr=0.0, momentum=0.0).setup(chain)       # lr 0: update() runs forward + backward and leaves the parameters alone
            opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
            torch.cuda.synchronize()
        finally:
            FPNMaskRCNNTrainChain.EARLY_RPN_BACKWARD = True
        res[early] = (float(chain.observation['loss']), m.ps.grads.clone(), m.ps)
    assert res[False][0] == res[True][0]
    ps = res[True][2]
    bad = []
    for name, (o, shape) in ps.offsets.items():
        n_ = int(np.prod(shape))
        a, c = res[False][1][o:o + n_], res[True][1][o:o + n_]
        if name.startswith('rpn/') or name.startswith('head/'):
            assert torch.equal(a, c), name
        elif name == 'extractor/resnet/conv1/b':
            continue            # a bias in front of a BatchNorm: its gradient is mathematically zero, what is stored is rounding noise
        else:
            scale = float(a.abs().max()) + 1e-30
            if float((a - c).abs().max()) > 1e-5 * scale:
                bad.append((name, float((a - c).abs().max()) / scale))
    assert not bad, sorted(bad, key=lambda t: -t[1])[:10]


def test_graphed_step_replays_the_eager_step():
    """optimizers.GraphedStep (bench.py --graph 1): the whole step - forward on three streams with the early RPN backward on the aux
    stream, backward with the filter gradients on the side stream, SGD - captured once into a HIP graph; replays must walk the same
    parameter trajectory as eager steps, bit for bit (sampler seeds live on the device and are advanced by the captured kernels)."""
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build('all')
        b = _batch()
        step_harness.seed(chain)
        opt = MomentumSGD(lr=1e-2, momentum=0.9, high_priority_stream=False).setup(chain)
        opt.add_hook(WeightDecay(0.0005))
        batch = [b['imgs'], b['bboxes'], b['labels'], b['masks']]
        if graphed:
            g = GraphedStep(opt, chain, batch, 1.0, warmup=3)
            for _ in range(2):
                g(*batch)
        else:
            for _ in range(5):
                opt.update(chain, *batch, 1.0)
        torch.cuda.synchronize()
        res.append((m.ps.params.clone(), float(chain.observation['loss'])))
    assert res[0][1] == res[1][1]
    assert torch.equal(res[0][0], res[1][0])


def test_laterals_off_the_chain_give_the_same_bits():
    """feature_pyramid_network.LATERALS_OFF_THE_CHAIN (off by default): the lateral 1x1 convolutions run beside the later ResNet stages in
    the forward pass and their data gradients beside the top-down chain of the backward pass - other streams, the same kernels on the same
    operands in the same summation order.  Losses, every gradient and the parameters after three updates must be the same bits."""
    from chainer_maskrcnn.model.extractor import feature_pyramid_network as fpn
    res = []
    for on in (False, True):
        fpn.LATERALS_OFF_THE_CHAIN = on
        try:
            m, chain = _build('all')
            b = _batch()
            step_harness.seed(chain)
            chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
            torch.cuda.synchronize()
            g, l = m.ps.grads.clone(), float(chain.observation['loss'])
            opt = MomentumSGD(lr=1e-2, momentum=0.9).setup(chain)
            opt.add_hook(WeightDecay(0.0005))
            for _ in range(3):
                opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
            torch.cuda.synchronize()
            res.append((l, g, m.ps.params.clone()))
        finally:
            fpn.LATERALS_OFF_THE_CHAIN = False
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])


def test_small_rpn_levels_beside_p2_give_the_same_bits():
    """multilevel_region_proposal_network.SMALL_LEVELS_BESIDE_P2 (off by default): the RPN convolutions of p3 .. p6 on the weight-gradient
    stream beside those of p2 - the same kernels on the same operands: same losses, gradients and parameters after three updates."""
    from chainer_maskrcnn.model.rpn import multilevel_region_proposal_network as rpn
    res = []
    for on in (False, True):
        rpn.SMALL_LEVELS_BESIDE_P2 = on
        try:
            m, chain = _build('all')
            b = _batch()
            step_harness.seed(chain)
            chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
            torch.cuda.synchronize()
            g, l = m.ps.grads.clone(), float(chain.observation['loss'])
            opt = MomentumSGD(lr=1e-2, momentum=0.9).setup(chain)
            opt.add_hook(WeightDecay(0.0005))
            for _ in range(3):
                opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
            torch.cuda.synchronize()
            res.append((l, g, m.ps.params.clone()))
        finally:
            rpn.SMALL_LEVELS_BESIDE_P2 = False
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize('arith', ['f32', 'bf16x6_behind_backbone'])
def test_composite_bottleneck_calls_give_the_same_bits(arith):
    """nn/core.py COMPOSITE_BLOCKS (on by default): one foreign call per ResNet bottleneck and pass (csrc/blocks.hip) enqueues the launches
    of the per-layer host path - same kernels, operands, order and streams.  Features, losses, every gradient and the parameters after
    three updates must be the same bits, in the float32 arithmetic and in the shipped one (forward split bracket of the backbone)."""
    from chainer_maskrcnn.nn import core
    res = []
    for on in (False, True):
        core.COMPOSITE_BLOCKS = on
        try:
            m = MaskRCNN(n_fg_class=80, device=DEV, seed=7, _test_shrink=dict(stages=STAGES, width_div=2))
            chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic=arith)
            chain.keep_outputs = True
            b = _batch()
            step_harness.seed(chain)
            chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
            torch.cuda.synchronize()
            feats = [f.clone() for f in chain.outputs['features']]
            g, l = m.ps.grads.clone(), float(chain.observation['loss'])
            stats = torch.cat([v.flatten() for _, v in sorted(m.ps.buffers.items())])       # BatchNorm running statistics
            opt = MomentumSGD(lr=1e-2, momentum=0.9).setup(chain)
            opt.add_hook(WeightDecay(0.0005))
            for _ in range(3):
                opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
            torch.cuda.synchronize()
            res.append((l, g, m.ps.params.clone(), feats, stats))
        finally:
            core.COMPOSITE_BLOCKS = True
    assert res[0][0] == res[1][0]
    for a, b_ in zip(res[0][3], res[1][3]):
        assert torch.equal(a, b_)
    assert torch.equal(res[0][4], res[1][4])
    assert torch.equal(res[0][1], res[1][1]) and float(res[0][1].abs().max()) > 0
    assert torch.equal(res[0][2], res[1][2])


def test_roi_align_backward_plans_built_beside_the_forward_give_the_same_bits():
    """fpn_roi_mask_head.PLAN_BWD_IN_FORWARD (opt-in): the entry lists of both ROIAlign backward calls are built on the weight-gradient
    stream during the forward pass and the backward follows them (mrcnn_roi_align_fpn_bwd_planned_f32) - the same bits as the fused backward:
    losses, every gradient, parameters after three updates."""
    from chainer_maskrcnn.model.head import fpn_roi_mask_head as hd
    res = []
    for on in (False, True):
        hd.PLAN_BWD_IN_FORWARD = on
        try:
            m, chain = _build('all')
            b = _batch()
            step_harness.seed(chain)
            chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
            torch.cuda.synchronize()
            g, l = m.ps.grads.clone(), float(chain.observation['loss'])
            opt = MomentumSGD(lr=1e-2, momentum=0.9).setup(chain)
            opt.add_hook(WeightDecay(0.0005))
            for _ in range(3):
                opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
            torch.cuda.synchronize()
            res.append((l, g, m.ps.params.clone()))
        finally:
            hd.PLAN_BWD_IN_FORWARD = False
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and float(res[0][1].abs().max()) > 0
    assert torch.equal(res[0][2], res[1][2])


def test_chain_puts_the_process_arithmetic_back_after_its_step():
    """a chain built with gemm_arithmetic selects it for ITS forward and backward pass and restores what it found at the end of
    backward() - an evaluation call or another model between two training steps keeps the process's own setting; a scaled loss after an
    early RPN backward is an error, not a silently wrong gradient."""
    from chainer_maskrcnn._hip import nn as hnn
    from chainer_maskrcnn.nn import core
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=7, _test_shrink=dict(stages=STAGES, width_div=2))
    chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, gemm_arithmetic='bf16x6_behind_backbone')
    b = _batch()
    assert tuple(hnn.split_operands()) == (0, 0, 0) and core.FWD_EMULATION_IN_BACKBONE is True
    loss = chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
    assert tuple(hnn.split_operands()) == (3, 3, 3) and core.FWD_EMULATION_IN_BACKBONE is False      # in force until the backward pass is done
    loss.backward()
    assert tuple(hnn.split_operands()) == (0, 0, 0) and core.FWD_EMULATION_IN_BACKBONE is True
    opt = MomentumSGD(lr=1e-3, momentum=0.9).setup(chain)
    opt.update(chain, b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
    assert tuple(hnn.split_operands()) == (0, 0, 0)
    # early RPN backward + a scaled loss
    chain.backward_follows = True
    try:
        chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)
    finally:
        chain.backward_follows = False
    with pytest.raises(RuntimeError, match='early'):
        chain.backward(upstream=torch.tensor(2.0, device=DEV))
