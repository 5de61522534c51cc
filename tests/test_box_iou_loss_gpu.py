"""GPU tests of the IoU box regression losses (csrc/box_loss.hip through ops.box_iou_loss): the kernel against
the float64 restatement tests/box_iou_loss_reference.py (pinned to torch float64 autograd by tests/test_box_iou_loss_cpu.py) at the
shapes where it can go wrong, the edge geometry, bit reproducibility, and the whole training step with the new arguments of
FPNMaskRCNNTrainChain.

Judged by tests/loss_judge.py: counts exact, the loss within 1e-5 of the float64 value, gradients element by element within
rtol * (|want| + weight * std_j / count) + FLT_MIN with rtol = 4 x max(the ratio of the reference's own float32 run on the same
inputs, 4 eps32); rows with label <= 0 exactly zero.  weight * std_j / count is the size of a gradient element whose box-space
derivative is 1: the sums of the chain rule cancel relative to it, not to the element.

Observed on an MI355X (largest elementwise gradient ratio over the cases of each kind, in eps32, against the bound of the case that gave
it; the float32 reference's own ratio is a quarter of the bound; the BOXRATIO lines this module prints):
  giou 247.0 of 988.2    diou 490.1 of 1960.4    ciou 490.1 of 1960.4    (all three at the 262147 rows against 1000 shared boxes)
  on the 600 random rows checked against autograd: giou 82.1 of 329.7, diou 130.4 of 520.4, ciou 130.4 of 520.4
  edge geometry and M = 1: at most 0.7 of 16
No case is above the float32 reference's own ratio by more than 0.6 %: the largest element is set by the rounding of the decoded
corners (a side of a few px at a coordinate near 1200 px), which both share, not by the kernel's expf / atanf.
Loss values: within 2.6e-7 of the float64 value everywhere (bar 1e-5).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'chainer-maskrcnn_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_keypoint_loss  # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay  # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch  # noqa: E402
import box_iou_loss_reference as ref  # noqa: E402
from loss_judge import EPS32, loss_close, ratio, rtol_from  # noqa: E402
from tests import step_harness  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('giou', 'diou', 'ciou')
MEAN, STD = ref.MEAN, ref.STD


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(x, t, rois, label, kind, ldx=4, col0=0, gfill=0, weight=1.0, roi_period=None, want_grad=True, mean=MEAN, std=STD, seed=0):
    """One ops.box_iou_loss call with the predictions in columns [col0, col0 + 4) of an (M, ldx) buffer of noise and a NaN-filled
    gradient buffer -> (loss_out (2,), the whole gradient buffer or None)."""
    M = x.shape[0]
    buf = np.random.RandomState(seed).standard_normal((M, ldx)).astype(np.float32)
    buf[:, col0:col0 + 4] = x
    gx = torch.full((M, ldx), float('nan'), dtype=torch.float32, device=DEV) if want_grad else None
    out, g = ops.box_iou_loss(_d(buf), ldx, _d(t), _d(rois), _d(label), M, kind, mean, std, weight=weight, roi_period=roi_period,
                              want_grad=want_grad, gfill=gfill, col0=col0, gx=gx)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (g.cpu().numpy() if want_grad else None)


def _judge(name, kind, got, x, t, rois, label, weight=1.0, roi_period=None, mean=MEAN, std=STD, rows=None):
    """loss_out and the (M,4) gradient against the float64 reference; ``rows``: compare the gradient on these rows only."""
    out, g = got
    loss, count, want = ref.box_iou_loss(x, t, rois, label, kind, mean, std, weight, roi_period)
    print('BOXLOSS %s %s got %.9g want %.9g rel %.3g' % (name, kind, out[0], loss, abs(float(out[0]) - loss) / max(abs(loss), 1e-6)))
    assert out[1] == count
    loss_close(out[0], loss)
    if g is None:
        return
    assert np.all(g[label <= 0] == 0)
    _, _, want32 = ref.box_iou_loss(x, t, rois, label, kind, mean, std, weight, roi_period, dtype=np.float32)
    extra = np.zeros_like(want)
    extra[label > 0] = weight * np.asarray(std, np.float64) / count
    if rows is not None:
        g, want, want32, extra = g[rows], want[rows], want32[rows], extra[rows]
    rtol = rtol_from(want32, want, extra)
    r = ratio(g, want, extra)
    print('BOXRATIO %s %s %.2f eps32 (bound %.2f eps32)' % (name, kind, r / EPS32, rtol / EPS32))
    assert r <= rtol, (name, kind, r / EPS32, rtol / EPS32)


_CACHE = {}


def _random(M, seed=0):
    """The tie-free random rows of tests/test_box_iou_loss_cpu.py (M = 600, seed 0 is the batch it checks against autograd)."""
    if (M, seed) not in _CACHE:
        x, t, rois, label = ref.make_inputs(M, seed)
        assert M == 0 or ref.row_gaps(x, t, rois).min() >= 1e-3
        _CACHE[M, seed] = (x, t, rois, label)
    return _CACHE[M, seed]


def _periodic(M, period, seed=1):
    """M rows against ``period`` shared boxes (the RPN's layout): targets and predictions drawn around the boxes, rows with a tie
    re-drawn, three quarters of the labels <= 0."""
    key = ('periodic', M, period, seed)
    if key not in _CACHE:
        rs = np.random.RandomState(seed)
        rois = ref.make_inputs(period, seed)[2]
        idx = np.arange(M) % period
        draw = lambda n: ((rs.standard_normal((n, 4)) * [3, 3, 1.5, 1.5]).astype(np.float32),
                          (rs.standard_normal((n, 4)) * 1.5).astype(np.float32))
        t, e = draw(M)
        x = t + e
        for _ in range(20):
            bad = np.nonzero(ref.row_gaps(x, t, rois[idx]) < 1e-3)[0]
            if not bad.size:
                break
            t[bad], e = draw(bad.size)
            x[bad] = t[bad] + e
        assert ref.row_gaps(x, t, rois[idx]).min() >= 1e-3
        label = np.where(rs.rand(M) < 0.25, rs.randint(1, 5, M), rs.randint(-1, 1, M)).astype(np.int32)
        label[-1] = 2                                   # the last row - only the wrapped iteration reaches it - counts
        _CACHE[key] = (x, t, rois, label)
    return _CACHE[key]


# ---- the kernel against the float64 reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M', [1, 257, 600])
def test_plain_layout_matches_float64(M, kind):
    """ldx = 4 (float4 loads and stores): one row, one row past a workgroup, the 600 rows checked against autograd on the CPU."""
    x, t, rois, label = _random(M, seed=0 if M == 600 else M)
    if M == 1:
        label = np.array([3], np.int32)
    _judge('plain M=%d' % M, kind, _run(x, t, rois, label, kind, weight=1.0 if M != 257 else 2.5), x, t, rois, label,
           weight=1.0 if M != 257 else 2.5)


@pytest.mark.parametrize('kind', KINDS)
def test_empty_call_writes_loss_0_count_1(kind):
    z = np.zeros((0, 4), np.float32)
    out, g = _run(z, z, np.zeros((1, 4), np.float32), np.zeros(0, np.int32), kind, roi_period=1)
    np.testing.assert_array_equal(out, np.array([0, 1], np.float32))
    assert g.shape == (0, 4)


@pytest.mark.parametrize('kind', KINDS)
def test_grid_stride_loop_partial_slots_and_roi_period(kind):
    """256 * 1024 + 3 rows against 1000 shared boxes: more rows than one pass of the 1024 x 256 grid covers, every partial slot in use,
    row r relative to rois[r % 1000]."""
    M, A = 256 * 1024 + 3, 1000
    x, t, rois, label = _periodic(M, A)
    assert rois.shape == (A, 4)
    got = _run(x, t, rois, label, kind, roi_period=A)
    _judge('wrap', kind, got, x, t, rois, label, roi_period=A)
    assert np.any(got[1][-1] != 0)


@pytest.mark.parametrize('kind', KINDS)
def test_head_layout_fills_its_columns_and_leaves_the_scores(kind):
    """ldx = 96, col0 = 88, gfill = 8 (the head's box_out row under the shrink) into a NaN-filled gradient: columns 88..91 receive the
    gradient, 92..95 zeros, 0..87 keep the fill bit for bit."""
    x, t, rois, label = _random(600)
    out, g = _run(x, t, rois, label, kind, ldx=96, col0=88, gfill=8, weight=10.0)
    assert np.isfinite(g[:, 88:]).all() and np.all(g[:, 92:] == 0)
    assert np.all(g[:, :88].view(np.uint32) == np.full((600, 88), np.nan, np.float32).view(np.uint32))
    _judge('head', kind, (out, g[:, 88:92]), x, t, rois, label, weight=10.0)


@pytest.mark.parametrize('kind', KINDS)
def test_unaligned_layout_takes_the_scalar_path(kind):
    """ldx = 7, col0 = 1, gfill = 6: neither the rows of x nor those of gx are 16-byte aligned; column 0 keeps the fill, 5 and 6 are zero."""
    x, t, rois, label = _random(257, seed=257)
    out, g = _run(x, t, rois, label, kind, ldx=7, col0=1, gfill=6)
    assert np.isnan(g[:, 0]).all() and np.all(g[:, 5:] == 0)
    _judge('scalar', kind, (out, g[:, 1:5]), x, t, rois, label)


@pytest.mark.parametrize('kind', KINDS)
def test_all_rows_ignored(kind):
    x, t, rois, _ = _random(600)
    for lab in (-1, 0):
        out, g = _run(x, t, rois, np.full(600, lab, np.int32), kind)
        np.testing.assert_array_equal(out, np.array([0, 1 if lab < 0 else 600], np.float32))
        assert np.all(g == 0)


@pytest.mark.parametrize('kind', KINDS)
def test_loss_only_call_gives_the_same_bits(kind):
    x, t, rois, label = _random(600)
    out, _ = _run(x, t, rois, label, kind)
    out2, g2 = _run(x, t, rois, label, kind, want_grad=False)
    assert g2 is None and out2.tobytes() == out.tobytes()
    _judge('loss only', kind, (out2, None), x, t, rois, label)


@pytest.mark.parametrize('kind', KINDS)
def test_two_calls_give_the_same_bits(kind):
    M, A = 256 * 1024 + 3, 1000
    x, t, rois, label = _periodic(M, A)
    a, b = _run(x, t, rois, label, kind, roi_period=A), _run(x, t, rois, label, kind, roi_period=A)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- edge geometry --------------------------------------------------------------------------------------------------------------------------
def _encode(gt, roi):
    """The targets.hip encoding of box gt against roi, normalised by MEAN / STD (float64)."""
    h, w = roi[2] - roi[0], roi[3] - roi[1]
    gh, gw = gt[2] - gt[0], gt[3] - gt[1]
    loc = np.array([(gt[0] + gh / 2 - roi[0] - h / 2) / h, (gt[1] + gw / 2 - roi[1] - w / 2) / w, np.log(gh / h), np.log(gw / w)])
    return (loc - np.asarray(MEAN)) / np.asarray(STD)


ROI = np.array([100., 200., 180., 300.])
_G = _encode(np.array([110., 190., 170., 310.]), ROI)
# name -> (x rows, t rows, roi rows, labels): a hand-written batch per case
EDGE = {
    'disjoint': ([_encode(np.array([300., 500., 340., 560.]), ROI)], [_G], [ROI], [1]),
    'prediction inside target': ([_encode(np.array([125., 215., 150., 280.]), ROI)], [_G], [ROI], [2]),
    'target inside prediction': ([_encode(np.array([90., 150., 200., 330.]), ROI)], [_G], [ROI], [2]),
    'identical': ([_G], [_G], [ROI], [1]),
    'dh = +80': ([np.array([0.3, -0.2, 80.0 / STD[2], 0.4])], [_G], [ROI], [1]),
    'dh = -80': ([np.array([0.3, -0.2, -80.0 / STD[2], 0.4])], [_G], [ROI], [1]),
    'zero-area roi': ([np.array([0.3, -0.2, 0.5, 0.4])], [np.array([0.1, 0.2, -0.3, 0.6])], [np.array([50., 60., 50., 60.])], [4]),
    'positive beside 0 and -1': ([_encode(np.array([120., 180., 190., 290.]), ROI)] * 3, [_G] * 3, [ROI] * 3, [0, 3, -1]),
}


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', list(EDGE))
def test_edge_geometry(case, kind):
    """Each case: counts exact, the loss within 1e-5 of the float64 reference, every gradient finite, rows with label <= 0 zero, and
    the gradient compared with the reference on the rows without a tie (ref.row_gaps >= 1e-3: the identical boxes, the zero-area
    prediction - whose overlap is 0 in float32 and 1e-33 px in float64 - and the zero-area RoI are ties).  Identical boxes: the
    float64 loss is at most eps / area, about 1e-11 - below what 1 - iou resolves in float32 - so the bar there is the absolute 1e-6."""
    x, t, rois = (np.asarray(v, np.float32) for v in EDGE[case][:3])
    label = np.asarray(EDGE[case][3], np.int32)
    out, g = _run(x, t, rois, label, kind)
    assert np.isfinite(out).all() and np.isfinite(g).all()
    loss, count, want = ref.box_iou_loss(x, t, rois, label, kind, MEAN, STD)
    print('BOXEDGE %s %s got %.9g want %.9g grad %s' % (case, kind, out[0], loss, g[label > 0][0]))
    assert out[1] == count == max(int((label >= 0).sum()), 1)
    if case == 'identical':
        assert 0 <= loss <= 1e-6 and abs(float(out[0])) <= 1e-6
    else:
        loss_close(out[0], loss)
    pos = np.nonzero(label > 0)[0]
    if case == 'disjoint':
        L, _ = ref.rows(x, t, rois, kind, MEAN, STD)
        assert L[0] > 1.0 and np.all(g[0, :2] != 0) and np.any(g[0, 2:] != 0)         # IoU 0, yet the box is pulled towards the target
    if case == 'dh = +80':
        assert g[0, 2] == 0 and want[0, 2] == 0 and g[0, 3] != 0
    if case == 'zero-area roi':
        assert np.all(g == 0)
    free = pos[ref.row_gaps(x[pos], t[pos], rois[pos]) >= 1e-3]
    assert (free.size == 0) == (case in ('identical', 'dh = -80', 'zero-area roi'))
    if free.size:
        _judge(case, kind, (out, g), x, t, rois, label, rows=free)
    assert np.all(g[label <= 0] == 0)


# ---- the whole step on the shrunk model ------------------------------------------------------------------------------------------------------
SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)


_batch, _forward, _step = step_harness.batch, step_harness.forward, step_harness.step


def _build(seed=7, **kw):
    return step_harness.build(SHRINK, seed, chain_kw=kw)


_SL1 = {}


def _smooth_l1_score_gradient():
    """The score columns of g_box of a smooth-L1 forward pass on the seeds of _forward (computed once)."""
    if not _SL1:
        m, chain = _build()
        _forward(chain, _batch())
        torch.cuda.synchronize()
        _SL1['g'] = chain.pending.g_box[:, :m.head.LOC0].clone()
    return _SL1['g']


@pytest.mark.parametrize('kind,weight,rpn_weight', [('giou', 1.0, 1.0), ('diou', 10.0, 0.5), ('ciou', 2.0, 3.0)])
def test_step_losses_equal_the_reference_on_the_step_own_tensors(kind, weight, rpn_weight):
    m, chain = _build(box_loss=kind, rpn_box_loss='giou', box_loss_weight=weight, rpn_box_loss_weight=rpn_weight)
    chain.keep_outputs = True
    b = _batch()
    _forward(chain, b)
    torch.cuda.synchronize()
    head = m.head
    g_box = chain.pending.g_box
    assert torch.equal(g_box[:, :head.LOC0], _smooth_l1_score_gradient())                # the classification gradient is untouched
    assert torch.isfinite(g_box).all() and bool((g_box[:, head.LOC0 + 4:] == 0).all())
    t = chain.targets
    box = chain.outputs['box'].cpu().numpy()[:, head.LOC0:head.LOC0 + 4]
    label = t['gt_roi_label'].cpu().numpy()
    assert (label > 0).sum() > 0
    want, _, _ = ref.box_iou_loss(box, t['gt_roi_loc'].cpu().numpy(), t['sample_roi'].cpu().numpy(), label, kind, chain.loc_normalize_mean,
                                  chain.loc_normalize_std, weight)
    loss_close(float(chain.observation['roi_loc_loss']), want)
    n, A = chain.rpn_targets[1].shape
    rl = chain.rpn_targets[1].reshape(-1).cpu().numpy()
    assert (rl > 0).sum() > 0
    want_rpn, _, _ = ref.box_iou_loss(chain.outputs['locs'].reshape(n * A, 4).cpu().numpy(), chain.rpn_targets[0].reshape(n * A, 4).cpu().numpy(),
                                      chain.rpn_out['anchors'].cpu().numpy(), rl, 'giou', weight=rpn_weight, roi_period=A)
    loss_close(float(chain.observation['rpn_loc_loss']), want_rpn)
    print('BOXSTEP %s roi_loc_loss %.6g (reference %.6g) rpn_loc_loss %.6g (reference %.6g)' % (
        kind, float(chain.observation['roi_loc_loss']), want, float(chain.observation['rpn_loc_loss']), want_rpn))
    chain.backward()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in chain.observation.values()), chain.observation
    g1 = m.ps.grads.clone()
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)                      # no float atomics: the same gradient buffer bit for bit


def test_defaults_are_untouched():
    """A chain built without the new arguments and one built with the smooth-L1 names spelled out: the same parameters and the same
    flat gradient buffer after one step, bit for bit."""
    res = []
    for kw in ({}, dict(box_loss='smooth_l1', rpn_box_loss='smooth_l1')):
        m, chain = _build(**kw)
        _step(chain, _batch())
        res.append((m.ps.params.clone(), m.ps.grads.clone(), {k: float(v) for k, v in chain.observation.items()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    assert float(res[0][1].abs().max()) > 0


def test_thirty_steps_reduce_the_loss():
    """The criterion of tests/test_groupnorm_gpu.py::test_thirty_steps_reduce_the_loss with box_loss='giou' at weight 1: 30 MomentumSGD
    steps (lr 0.01, momentum 0.9, weight decay 5e-4) on one fixed batch, every loss finite, the total loss at least halves between its
    first and last five steps.  The roi_loc_loss trajectory is printed, not asserted."""
    m, chain = _build(seed=11, box_loss='giou', box_loss_weight=1.0)
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
    print('BOXTRAJECTORY roi_loc_loss', ' '.join('%.4f' % v for v in h[:, 2]))
    assert last[5] <= 0.5 * first[5], (first, last)
    assert torch.isfinite(m.ps.params).all()


def test_keypoint_chain_runs_one_step():
    K = 17
    m = MaskRCNN(n_fg_class=1, n_keypoints=K, head_arch='fpn_keypoint', device=DEV, seed=11, _test_shrink=SHRINK)
    chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_keypoint_loss, binary_mask=False, box_loss='ciou')
    b = make_batch(5, 2, 128, 160, G=3, n_fg_class=1, n_keypoints=K)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
    b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    chain(b['imgs'], b['bboxes'], b['labels'], b['keypoints'], 1.0).backward()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in chain.observation.values())
    assert float(chain.observation['roi_loc_loss']) > 0
    assert torch.isfinite(m.ps.grads).all()


def test_graphed_step_replays_the_eager_step():
    """optimizers.GraphedStep with both box losses on GIoU: captured once (after 3 eager warm-up steps), one replay - the parameters of
    four eager steps, bit for bit (no host synchronisation and no allocation inside the call)."""
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build(box_loss='giou', rpn_box_loss='giou')
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
