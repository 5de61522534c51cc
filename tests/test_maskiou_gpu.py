"""Mask Scoring R-CNN on the GPU (csrc/maskiou.hip, MaskIoUHead, the training chain and inference) against
tests/maskiou_reference.py.  The integer counts equal the reference's on every row; the target equals the float32 restatement bit for bit;
input assembly, its backward and the rescoring equal NumPy bit for bit; the loss is judged against float64 as tests/loss_judge.py does."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskiou_reference as mr            # noqa: E402
from loss_judge import EPS32, loss_close, ratio, rtol_from            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = mr.target_cases()
I32 = torch.int32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _target(c, label_base=1, counts=True):
    from chainer_maskrcnn._hip import ops
    o = ops.maskiou_target(_t(c['masks']), _t(c['n_gt']), _t(c['sample_roi']), _t(c['gt_assign']), _t(c['label']), _t(c['n_pos']), c['n_sample'],
                           c['rows'], _t(c['mask_out']), _t(c['gt_roi_mask']), c['n_fg'], label_base=label_base, want_counts=counts)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---- the target kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,case', CASES, ids=[c[0] for c in CASES])
def test_target_counts_and_value(name, case):
    """The bound against float64.  Every count is an integer below 2^24, so its conversion is exact, and with u = 2^-24 = eps32 / 2:
    full_est = fl(fl(gt28 * full) / crop) carries two roundings, a relative error <= 2u.  uni = fl(fl(pred + full_est) - ovr): since
    ovr <= pred <= uni and full_est = uni + ovr - pred <= 2 uni, the absolute error is at most 2u full_est + u (pred + full_est) + u uni
    <= 4u uni + 2u uni + u uni = 7u uni.  fmaxf is exact (uni < 1 only where ovr = 0, a zero target either way), the last division adds u:
    |target32 - target64| <= 8u target + O(u^2) = 4 eps32 target; the test takes 4.5 eps32 for the second-order terms and float64's own
    rounding.  The float32 restatement rounds exactly as the kernel does - exact integers in, a fixed operation order, correctly rounded
    division - so against it there is no freedom: bit equality."""
    got = _target(case)
    want = mr.target_counts(case)
    assert got['counts'].dtype == np.int32 and got['area'].dtype == np.int32 and got['target'].dtype == np.float32
    np.testing.assert_array_equal(got['area'], mr.mask_areas(case['masks'], case['n_gt']))
    np.testing.assert_array_equal(got['counts'], want)
    t32, t64 = mr.target_from_counts(want, np.float32), mr.target_from_counts(want, np.float64)
    np.testing.assert_array_equal(got['target'], t32)
    err = np.abs(got['target'].astype(np.float64) - t64)
    print('%s: target max err %.2f eps32 of the target, %d rows > 0' % (name, float((err / np.maximum(t64, 1e-300)).max() / EPS32), int((t64 > 0).sum())))
    assert (err <= 4.5 * EPS32 * t64).all()
    assert (got['target'] > 0).any() and (got['target'] == 0).any()
    np.testing.assert_array_equal(_target(case, counts=False)['target'], t32)           # the counts are optional


@pytest.mark.parametrize('H,W,n_fg', [(37, 45, 3), (64, 64, 80)])
def test_target_ignores_the_unused_mask_slots_and_knows_its_edges(H, W, n_fg):
    a, z = _target(mr.edge_case(H, W, n_fg, junk=255)), _target(mr.edge_case(H, W, n_fg, junk=0))
    for k in a:
        np.testing.assert_array_equal(a[k], z[k], err_msg=k)
    assert not a['area'][0, 3] and not a['area'][1].any() and a['area'][0, 0] == 15 * 23 - 16
    row = dict(zip(mr.EDGE_ROWS, range(12)))
    t = a['target']
    assert t[row['exact one']] == np.float32(1.0)
    for k in ('no integer extent', 'all-zero mask', 'crop 0, full > 0', 'all logits negative', 'behind n_pos', 'no assignment', 'background'):
        assert t[row[k]] == 0, k
    for k in ('partly outside', 'the image', 'last channel', 'ordinary'):
        assert 0 < t[row[k]] <= 1, k
    assert not t[12:].any() and not a['counts'][9:].any()           # n_pos = 0: an image without positives


def test_target_with_zero_based_labels_and_without_rows():
    from chainer_maskrcnn._hip import ops
    c = mr.random_case(5, 37, 45, 3)
    shifted = dict(c, label=(c['label'] - 1).astype(np.int32))
    np.testing.assert_array_equal(_target(shifted, label_base=0)['counts'], _target(c)['counts'])
    e = mr.edge_case(37, 45, 3)
    o = ops.maskiou_target(_t(e['masks']), _t(e['n_gt']), _t(e['sample_roi']), _t(e['gt_assign']), torch.zeros((0,), dtype=I32, device=DEV),
                           _t(e['n_pos']), 12, 0, torch.zeros((0, 28, 28, 32), device=DEV), torch.zeros((0, 28, 28), dtype=I32, device=DEV), 3,
                           want_counts=True)
    torch.cuda.synchronize()
    assert o['target'].shape == (0,) and o['counts'].shape == (0, 5)
    with pytest.raises(ValueError):
        ops.maskiou_target(_t(e['masks']), _t(e['n_gt']), _t(e['sample_roi']), _t(e['gt_assign']), _t(e['label'][:5]), _t(e['n_pos']), 12, 12,
                           _t(e['mask_out']), _t(e['gt_roi_mask']), 3)


# ---- input assembly, loss, rescoring ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,n_fg', [(64, 3), (256, 80)])
def test_input_assembly_and_its_backward_equal_numpy(C, n_fg):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(C)
    Rm, Cp, cin_p = 5, mr.pad32(n_fg), C + 32
    feat = rs.standard_normal((Rm, 14, 14, C)).astype(np.float32)
    logit = (rs.standard_normal((Rm, 28, 28, Cp)) * 3).astype(np.float32)
    label = np.array([1, n_fg, 0, 2, -1], np.int32)             # the first and the last channel, a background row, a padding row
    got = ops.maskiou_input_fwd(_t(feat), _t(logit), _t(label), n_fg, cin_p)
    want = mr.input_fwd(feat, logit, label, cin_p)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert not want[2, :, :, C].any() and not want[4, :, :, C].any() and want[1, :, :, C].any() and not want[..., C + 1:].any()
    base0 = ops.maskiou_input_fwd(_t(feat), _t(logit), _t(np.maximum(label - 1, -1).astype(np.int32)), n_fg, cin_p, label_base=0)
    np.testing.assert_array_equal(base0.cpu().numpy(), want)
    # backward: one add per element of the first C channels; a larger buffer behind g_pool shows that nothing beyond it is touched
    g_in = rs.standard_normal((Rm, 14, 14, cin_p)).astype(np.float32)
    g_pool = rs.standard_normal((Rm, 14, 14, C)).astype(np.float32)
    buf = torch.full((g_pool.size + 1024,), 7.0, device=DEV)
    view = buf[:g_pool.size].view(Rm, 14, 14, C)
    view.copy_(_t(g_pool))
    out = ops.maskiou_input_bwd(_t(g_in), view)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    np.testing.assert_array_equal(view.cpu().numpy(), mr.input_bwd(g_in, g_pool))
    assert bool((buf[g_pool.size:] == 7.0).all())
    empty = ops.maskiou_input_fwd(torch.zeros((0, 14, 14, C), device=DEV), torch.zeros((0, 28, 28, Cp), device=DEV),
                                  torch.zeros((0,), dtype=I32, device=DEV), n_fg, cin_p)
    assert empty.shape == (0, 14, 14, cin_p)


@pytest.mark.parametrize('Rm,n_fg,weight', [(16, 3, 1.0), (128, 80, 1.0), (128, 80, 2.5), (1500, 80, 0.3)])
def test_l2_loss_against_float64(Rm, n_fg, weight):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(Rm + n_fg)
    ld = mr.pad32(n_fg)
    pred = rs.standard_normal((Rm, ld)).astype(np.float32)
    tgt = np.where(rs.rand(Rm) < 0.6, rs.rand(Rm), 0.0).astype(np.float32)
    label = rs.randint(1, n_fg + 1, Rm).astype(np.int32)
    label[::7] = 0                              # background rows carry no target in the chain; here some do, and are skipped
    label[-1], tgt[-1] = n_fg, 0.5              # the last logical channel
    out, gx = ops.maskiou_l2(_t(pred), _t(tgt), _t(label), n_fg, weight=weight)
    torch.cuda.synchronize()
    out, gx = out.cpu().numpy(), gx.cpu().numpy()
    w_loss, w_count, w_gx = mr.l2(pred, tgt, label, weight, dtype=np.float64)
    f_loss, _, f_gx = mr.l2(pred, tgt, label, weight, dtype=np.float32)
    rl, rg = rtol_from(np.array([f_loss]), np.array([w_loss])), rtol_from(f_gx, w_gx)
    print('l2 Rm %d: loss %.1f eps32 (bar %.1f), gradient %.1f eps32 (bar %.1f)' % (Rm, ratio(out[:1], [w_loss]) / EPS32, rl / EPS32,
                                                                                    ratio(gx, w_gx) / EPS32, rg / EPS32))
    assert out[1] == w_count and w_count > 4
    assert ratio(out[:1], np.array([w_loss])) <= rl and ratio(gx, w_gx) <= rg
    off = np.ones_like(gx, bool)
    rows = np.nonzero((tgt > 0) & (label > 0))[0]
    off[rows, label[rows] - 1] = False
    assert not gx[off].any() and gx[~off].all()                # zero off the label column and in every row without a target
    # without the gradient, and two runs give the same bits
    out2, none = ops.maskiou_l2(_t(pred), _t(tgt), _t(label), n_fg, weight=weight, want_grad=False)
    assert none is None and torch.equal(out2.cpu(), torch.from_numpy(out))


def test_l2_loss_without_any_target_is_zero():
    from chainer_maskrcnn._hip import ops
    pred = torch.randn((40, 32), device=DEV)
    label = torch.randint(0, 4, (40,), dtype=I32, device=DEV)
    gx = torch.full((40, 32), 3.0, device=DEV)
    out, g = ops.maskiou_l2(pred, torch.zeros((40,), device=DEV), label, 3, gx=gx)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 1.0] and g is gx and not bool(gx.any())          # mrcnn_loss_total_f32 adds the 0 whatever the count is
    out, g = ops.maskiou_l2(torch.zeros((0, 32), device=DEV), torch.zeros((0,), device=DEV), torch.zeros((0,), dtype=I32, device=DEV), 3)
    assert out.cpu().tolist() == [0.0, 1.0] and g.shape == (0, 32)


def test_rescore_equals_numpy():
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(2)
    D, ld = 300, 96
    pred = (rs.standard_normal((D, ld)) * 0.8 + 0.5).astype(np.float32)
    label = rs.randint(0, 80, D).astype(np.int32)
    label[:2] = (0, 79)
    score = rs.rand(D).astype(np.float32)
    picked = pred[np.arange(D), label]
    assert (picked < 0).any() and (picked > 1).any() and ((picked > 0) & (picked < 1)).any()
    got = ops.maskiou_rescore(_t(score), _t(pred), _t(label), 80)
    np.testing.assert_array_equal(got.cpu().numpy(), mr.rescore(score, pred, label))
    assert ops.maskiou_rescore(torch.zeros((0,), device=DEV), torch.zeros((0, ld), device=DEV), torch.zeros((0,), dtype=I32, device=DEV), 80).shape == (0,)


# ---- the model, the training chain and inference ------------------------------------------------------------------------------------------
from chainer_maskrcnn.model.head.fpn_roi_mask_head import roi_align_fpn_bwd            # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN            # noqa: E402
from chainer_maskrcnn.nn import core            # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay            # noqa: E402
from tests import step_harness            # noqa: E402

SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
D64 = torch.float64
SIX = {'rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss'}


_build, _batch, _check = functools.partial(step_harness.build, SHRINK), step_harness.batch, step_harness.check
_forward, _step = step_harness.forward, step_harness.step
_predict_model = functools.partial(step_harness.predict_model, SHRINK)


def _own(m):
    return [n for n in m.ps.names() if n.startswith('head/maskiou/')]


def test_defaults_are_untouched():
    """mask_iou=False and a model built without the argument: the same offsets, parameters and flat gradient buffer, bit for bit, and
    exactly today's six observation keys."""
    res = []
    for kw in ({}, {'mask_iou': False}):
        m, chain = _build(**kw)
        _step(chain, _batch())
        assert m.maskiou_head is None and m.head.last_mask_pool is None and chain.observation.keys() == SIX
        res.append((m.ps.params.clone(), m.ps.grads.clone(), dict(m.ps.offsets)))
    assert res[0][2] == res[1][2] and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0


@pytest.mark.parametrize('H,W', [(14, 14), (15, 9)])
def test_strided_3x3_layer_backward_against_float64(H, W):
    """conv4 of the head: Conv.bwd of a 3x3 / 2 layer (gy scattered onto the stride-1 lattice, then the stride-1 data gradient) and its
    filter gradient against torch's float64 autograd on the CPU, the ReLU masks of both sides included."""
    import torch.nn.functional as F
    from chainer_maskrcnn.nn.core import Conv, ParamStore
    ps = ParamStore()
    cv = Conv(ps, 't/conv4', 64, 64, 3, 2, 1, relu=True)
    ps.materialise(torch.device(DEV), 3)
    g = torch.Generator().manual_seed(H * W)
    x = torch.relu(torch.randn((3, H, W, 64), generator=g))           # the layer's input is a ReLU output
    gy = torch.randn((3, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), generator=g)
    y, tape = cv.fwd(x.to(DEV))
    gy = gy * (y.cpu() > 0)                                             # masked by the layer above, as in MaskIoUHead.backward
    gx = cv.bwd(tape, gy.to(DEV).contiguous(), gy_masked=True, mask_gx=True)
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    bad = []
    ref = {}
    for dt in (D64, torch.float32):
        xr = x.to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        w = cv.W.cpu().to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        out = F.conv2d(xr, w, cv.b.cpu().to(dt), stride=2, padding=1)
        (out * gy.to(dt).permute(0, 3, 1, 2)).sum().backward()
        ref[dt] = (out.detach().clamp(min=0).permute(0, 2, 3, 1), (xr.grad * (xr > 0)).permute(0, 2, 3, 1), w.grad.permute(0, 2, 3, 1))
    _check('3x3/2 forward', y, ref[D64][0], ref[torch.float32][0], bad)
    _check('3x3/2 data gradient', gx, ref[D64][1], ref[torch.float32][1], bad)
    _check('3x3/2 filter gradient', ps.g('t/conv4/W'), ref[D64][2], ref[torch.float32][2], bad)
    assert not bad, bad
    assert float(gx.abs().max()) > 0 and not bool(gx[x.to(DEV) <= 0].any())


@pytest.mark.parametrize('mask_rows', ['all', 'positives'])
def test_wiring(mask_rows):
    from chainer_maskrcnn._hip import ops
    m, chain = _build(mask_iou=True, mask_rows=mask_rows, chain_kw=dict(mask_iou_weight=1.5))
    chain.EARLY_RPN_BACKWARD = False
    chain.keep_outputs = True
    b = _batch()
    _step(chain, b)
    out, t, head, mh = chain.outputs, chain.targets, m.head, m.maskiou_head
    iou = out['maskiou']
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert obs.keys() == SIX | {'maskiou_loss'} and all(np.isfinite(v) for v in obs.values())
    S, rows = chain.proposal_target_creator.n_sample, t['mask_rows']
    assert rows == (S if mask_rows == 'all' else chain.proposal_target_creator.pos_cap)
    m_label = chain.mask_inputs[2].contiguous()
    n_gt = ops.count_valid_labels(b['labels'].to(I32).contiguous())
    C = head.channels
    # (a) the kept target = a direct call of the target kernel on the kept tensors, and the NumPy reference on them
    again = ops.maskiou_target(b['masks'].contiguous(), n_gt, t['sample_roi'], t['gt_assign'], m_label, t['n_pos'], S, rows, out['mask'],
                               t['gt_roi_mask'], 80, want_counts=True)
    for k in ('target', 'area', 'counts'):
        assert torch.equal(again[k], iou[k]), k
    assert bool((iou['target'] > 0).any()) and bool((iou['target'] <= 1).all())
    case = dict(masks=b['masks'].cpu().numpy(), n_gt=n_gt.cpu().numpy(), sample_roi=t['sample_roi'].cpu().numpy(), gt_assign=t['gt_assign'].cpu().numpy(),
                label=m_label.cpu().numpy(), n_pos=t['n_pos'].cpu().numpy(), n_sample=S, rows=rows, mask_out=out['mask'].cpu().numpy(),
                gt_roi_mask=t['gt_roi_mask'].cpu().numpy())
    counts = mr.target_counts(case)
    np.testing.assert_array_equal(iou['counts'].cpu().numpy(), counts)
    np.testing.assert_array_equal(iou['target'].cpu().numpy(), mr.target_from_counts(counts, np.float32))
    # the head's input = the assembly kernel on the kept pooled features and logits
    assert torch.equal(iou['input'], ops.maskiou_input_fwd(out['mask_pool'], out['mask'], m_label, 80, mh.cin_p))
    np.testing.assert_array_equal(iou['input'].cpu().numpy(), mr.input_fwd(out['mask_pool'].cpu().numpy(), case['mask_out'], case['label'], mh.cin_p))
    # (b) the loss and its gradient on the kept prediction and target
    pred, tgt = iou['pred'].cpu().numpy(), iou['target'].cpu().numpy()
    w_loss, w_count, w_gx = mr.l2(pred, tgt, case['label'], 1.5, dtype=np.float64)
    loss_close(obs['maskiou_loss'], w_loss)
    rows_l = out['losses'].cpu().numpy()
    assert rows_l.shape == (6, 2) and rows_l[5, 1] == w_count and float(rows_l[5, 0]) == obs['maskiou_loss']
    total = np.float32(0)
    for v in rows_l[:, 0]:
        total = np.float32(total + v)
    assert np.float32(obs['loss']) == total
    assert ratio(iou['g_pred'].cpu().numpy(), w_gx) <= rtol_from(mr.l2(pred, tgt, case['label'], 1.5, dtype=np.float32)[2], w_gx)
    # (c) the head's forward on the kept input against float64
    params = {n: m.ps.p(n).cpu().numpy() for n in _own(m)}
    x = iou['input'].cpu().numpy()
    bad = []
    _check('maskiou head forward', iou['pred'], torch.from_numpy(mr.head_forward(params, x, np.float64)),
           torch.from_numpy(mr.head_forward(params, x, np.float32)), bad)
    # (e) the pyramid gradient behind the heads = the box part + ONE ROIAlign backward of (mask convs' pooled gradient + the head's feature gradient)
    pooled = out['g_mask_pool_convs'] + out['g_maskiou_in'][..., :C]
    assert torch.equal(out['g_mask_pool'], pooled) and float(out['g_maskiou_in'][..., :C].abs().max()) > 0
    bufs = [torch.empty_like(f) for f in out['features']]
    roi_align_fpn_bwd(pooled.contiguous(), bufs, chain.mask_inputs[0], chain.mask_inputs[1], head.roi_size_mask, m.extractor.spatial_scales,
                      accumulate=False)
    torch.cuda.synchronize()
    for l in range(len(out['features'])):
        box, part = out['g_feats_box'][l].cpu(), bufs[l].cpu()
        _check('pyramid gradient level %d' % l, out['g_feats_heads'][l], box.to(D64) + part.to(D64), box + part, bad)
    assert not bad, bad
    # (d) the head/maskiou/ gradients = the head alone on the kept input and loss gradient, bit for bit
    kept = {n: m.ps.g(n).clone() for n in m.ps.names()}
    m.ps.grads.zero_()
    assert torch.equal(mh.forward(iou['input']), iou['pred'])
    g_in = mh.backward(iou['g_pred'])
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    assert torch.equal(g_in, out['g_maskiou_in'])
    for n in _own(m):
        assert torch.equal(m.ps.g(n), kept[n]) and float(kept[n].abs().max()) > 0 and torch.isfinite(kept[n]).all(), n
    # (f), (g) against the same step with mask_iou off: the mask logits' gradient (the logit channel is a constant) and every parameter
    # gradient outside head/maskiou/, outside the mask convolutions and outside what lies below the pooled features, bit for bit
    m0, chain0 = _build(mask_rows=mask_rows)
    chain0.EARLY_RPN_BACKWARD = False
    loss0 = _forward(chain0, b)
    g_mask0 = chain0.pending.g_mask.clone()
    loss0.backward()
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    assert torch.equal(out['g_mask'], g_mask0) and float(g_mask0.abs().max()) > 0
    mask_convs = tuple(cv.name + '/' for cv in head.mask_convs)
    same = [n for n in m0.ps.names() if (n.startswith('head/') or n.startswith('rpn/')) and not n.startswith(mask_convs)]
    assert 'head/fc1/W' in same and 'head/deconv1/W' in same and 'head/conv2/W' in same and 'rpn/conv/W' in same and 'head/mask1/W' not in same
    for n in same:
        assert torch.equal(kept[n], m0.ps.g(n)), n
    for k in SIX - {'loss'}:
        assert obs[k] == float(chain0.observation[k]), k


def test_step_is_finite_and_bit_reproducible():
    m, chain = _build(mask_iou=True)
    b = _batch()
    _step(chain, b)
    g1 = m.ps.grads.clone()
    assert torch.isfinite(g1).all()
    assert len(_own(m)) == 14
    for n in _own(m):
        g = m.ps.g(n)
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, n
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)                      # no float atomics anywhere in the new path


@pytest.mark.parametrize('kw', [dict(cascade_ious=(0.5, 0.6, 0.7)), dict(head_norm='gn', gn_groups=16)], ids=['cascade', 'gn'])
def test_step_with_cascade_and_with_groupnorm(kw):
    m, chain = _build(mask_iou=True, **kw)
    chain.keep_outputs = True
    b = _batch()
    _step(chain, b)
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert all(np.isfinite(v) for v in obs.values()) and obs['maskiou_loss'] > 0, obs
    rows = chain.outputs['losses'].cpu().numpy()
    assert rows.shape[0] == 6 + 2 * len(m.cascade_heads) and float(rows[-1, 0]) == obs['maskiou_loss']         # behind the cascade's rows
    g1 = m.ps.grads.clone()
    assert torch.isfinite(g1).all() and all(float(m.ps.g(n).abs().max()) > 0 for n in _own(m))
    assert not any('/gn/' in n for n in _own(m))
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)


def test_upstream_scales_the_new_seed_like_the_others():
    m, chain = _build(mask_iou=True)
    b = _batch()
    _step(chain, b)
    g1 = {n: m.ps.g(n).clone() for n in _own(m)}
    _forward(chain, b)
    chain.backward(upstream=torch.tensor(2.0, device=DEV))
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    for n, g in g1.items():            # a power of two scales every product and sum exactly
        assert torch.equal(m.ps.g(n), g * 2), n


def test_grad_ready_hook_sees_final_maskiou_gradients():
    m, chain = _build(mask_iou=True)
    b = _batch()
    _step(chain, b)
    want = m.ps.grads.clone()
    first = m.ps.offsets['head/maskiou/conv1/W'][0]
    assert first == min(m.ps.offsets[n][0] for n in _own(m)) and first > max(o for n, (o, _) in m.ps.offsets.items() if not n.startswith('head/maskiou/'))
    seen, snap = [], {}

    def hook(offset):
        seen.append(offset)
        if offset <= first and not snap:
            core.join_side_stream(torch.device(DEV))
            torch.cuda.synchronize()
            snap.update({n: m.ps.g(n).clone() for n in _own(m)})
    m.ps.grads.zero_()
    chain.grad_ready_hook = hook
    _step(chain, b)
    chain.grad_ready_hook = None
    assert torch.equal(m.ps.grads, want)                    # the hook changes nothing
    assert seen[0] == chain._offset_of('head/') <= first and seen[-1] == 0 and snap
    for n, g in snap.items():                               # at the first report every parameter at or above the offset is final
        assert torch.equal(g, m.ps.g(n)) and float(g.abs().max()) > 0, n


def test_thirty_steps_reduce_the_loss():
    """The criterion and optimizer settings of tests/test_cascade_gpu.py::test_thirty_steps_reduce_the_loss with the MaskIoU head; nothing
    is asserted about the trend of maskiou_loss itself (its first and last values are printed, and recorded in DESIGN.md section 3.22)."""
    m, chain = _build(seed=11, mask_iou=True)
    opt = MomentumSGD(lr=0.01, momentum=0.9).setup(chain)
    opt.add_hook(WeightDecay(0.0005))
    b = _batch()
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss', 'maskiou_loss')
    w0 = m.ps.p('head/maskiou/fc2/W').clone()
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
    print('maskiou_loss first step %.6f, last step %.6f' % (h[0, 6], h[-1, 6]))
    assert last[5] <= 0.5 * first[5], (first, last)
    assert torch.isfinite(m.ps.params).all()
    assert not torch.equal(w0, m.ps.p('head/maskiou/fc2/W'))


def test_graphed_step_replays_the_eager_step():
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build(mask_iou=True)
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
        res.append((m.ps.params.clone(), float(chain.observation['loss']), float(chain.observation['maskiou_loss'])))
    assert res[0][1:] == res[1][1:]
    assert torch.equal(res[0][0], res[1][0])


def test_predict_rescoring(tmp_path):
    from chainer_maskrcnn._hip import ops
    from chainer_maskrcnn.utils.chainer_npz import load_npz, save_npz
    m = _predict_model(5, mask_iou=True)
    bias = m.ps.p('head/maskiou/maskiou/b')         # freshly initialised outputs are near 0: move them to about -0.5, 0.5 and 0.75 by class
    bias[:80].copy_(torch.tensor([-0.5, 0.5, 0.75], device=DEV).repeat(27)[:80])         # (the padded outputs stay zero: a file holds the 80)
    rs = np.random.RandomState(0)
    imgs = [torch.from_numpy((rs.rand(3, h, w) * 255).astype(np.float32)) for h, w in ((120, 150), (100, 100))]
    kept = []
    for img in imgs:
        masks, labels, scores = m.predict([img])
        x_in, pred = m.last_maskiou
        kept.append((masks[0], labels[0], scores[0], m.last_bboxes[0], m.last_box_scores[0], pred.clone()))
    assert m.train is True and core.TRAIN is True
    both = m.predict(imgs)
    m.mask_iou_rescore = False
    plain = m.predict(imgs)
    plain_boxes, plain_box_scores = m.last_bboxes, m.last_box_scores
    m.mask_iou_rescore = True
    for i, (mask, label, score, bbox, box_score, pred) in enumerate(kept):
        D = label.shape[0]
        assert D > 0 and pred.shape == (D, m.maskiou_head.out_p)
        # order, count, masks, labels and boxes are those of the box scores
        assert torch.equal(mask, plain[0][i]) and torch.equal(label, plain[1][i]) and torch.equal(bbox, plain_boxes[i])
        assert torch.equal(box_score, plain[2][i]) and torch.equal(box_score, plain_box_scores[i])
        iou = pred.cpu().numpy()[np.arange(D), label.cpu().numpy()]
        want = box_score.cpu().numpy() * np.fmin(np.fmax(iou, np.float32(0)), np.float32(1))
        np.testing.assert_array_equal(score.cpu().numpy(), want)
        assert torch.equal(score, ops.maskiou_rescore(box_score.contiguous(), pred, label.to(I32).contiguous(), 80))
        for k in range(3):                                  # an image's result does not depend on its batch neighbours
            assert torch.equal(both[k][i], (mask, label, score)[k])
        assert not torch.equal(score, box_score) and bool((score <= box_score).all())
    # the cap acts on the box scores, before the rescoring
    m.use_max_detections(5)
    capped = m.predict(imgs[:1])
    m.mask_iou_rescore = False
    capped_plain = m.predict(imgs[:1])
    m.mask_iou_rescore = True
    m.use_max_detections(None)
    assert 0 < capped[1][0].shape[0] <= 5 and torch.equal(capped[1][0], capped_plain[1][0]) and torch.equal(capped[0][0], capped_plain[0][0])
    # the npz round trip
    path = str(tmp_path / 'maskiou.npz')
    save_npz(path, m)
    fresh = _predict_model(6, mask_iou=True)
    assert not torch.equal(fresh.ps.params, m.ps.params)
    load_npz(path, fresh, strict=True)
    assert torch.equal(fresh.ps.params, m.ps.params)
    again = fresh.predict(imgs[:1])
    for k in range(3):
        assert torch.equal(again[k][0], kept[0][k])
    # a plain model's file fills everything but the MaskIoU head; strict refuses it
    p = _predict_model(8)
    assert p.predict(imgs[:1])[1][0].shape[0] > 0 and p.last_maskiou is None and torch.equal(p.last_box_scores[0], p.predict(imgs[:1])[2][0])
    ppath = str(tmp_path / 'plain.npz')
    save_npz(ppath, p)
    other = _predict_model(9, mask_iou=True)
    init = {n: other.ps.p(n).clone() for n in _own(other)}
    load_npz(ppath, other, strict=False)
    for n in p.ps.names():
        assert torch.equal(other.ps.p(n), p.ps.p(n)), n
    for n, v in init.items():
        assert torch.equal(other.ps.p(n), v), n
    with pytest.raises(KeyError):
        load_npz(ppath, other, strict=True)
    with pytest.raises(ValueError):
        m.use_test_augmentation([160, 200])


def test_refusals_on_the_device():
    with pytest.raises(ValueError, match='mask_iou'):
        MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', device=DEV, _test_shrink=SHRINK, mask_iou=True)
    for arch, backbone in (('res5', 'c4'), ('light', 'fpn')):
        with pytest.raises(ValueError, match='mask_iou'):
            MaskRCNN(n_fg_class=5, backbone=backbone, head_arch=arch, device=DEV, _test_shrink=dict(width_div=4) if arch == 'res5' else SHRINK,
                     mask_iou=True)
