"""The Cascade R-CNN kernels (csrc/cascade.hip) on the GPU against tests/cascade_reference.py: the stage-to-stage
step on the fixed random geometries (integer outputs equal on every row - tests/test_cascade_cpu.py shows that no row of these cases is
within 1e-5 of a decision boundary, so nothing is exempt; boxes and targets judged against float64 as tests/loss_judge.py does), its edges
in exact arithmetic, and the inference score."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cascade_reference as cr            # noqa: E402
from loss_judge import EPS32, ratio, rtol_from            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INT_KEYS = ('label', 'gt_assign', 'levels')
FLOAT_KEYS = ('roi', 'rois_xy5', 'gt_loc')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _refine(case, thr, sp, sn, size, train=True, prev=True):
    from chainer_maskrcnn._hip import ops
    kw = dict(gt_boxes=_t(case['gt_boxes']), gt_labels=_t(case['gt_labels']), n_gt=_t(case['n_gt']), iou_thresh=thr, std_next=sn) if train else {}
    out = ops.cascade_refine(_t(case['rois']), _t(case['box_out']), cr.LOC0, case['N'], cr.MEAN, sp, _t(size) if isinstance(size, np.ndarray) else size,
                             prev_label=_t(case['prev_label']) if prev else None, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_CASES = cr.random_cases()


@pytest.mark.parametrize('name,case,thr,sp,sn,size', _CASES, ids=[c[0] for c in _CASES])
def test_refine_matches_the_reference_on_random_rows(name, case, thr, sp, sn, size):
    got = _refine(case, thr, sp, sn, size)
    want = cr.run_case(case, thr, sp, sn, size, np.float64)
    f32 = cr.run_case(case, thr, sp, sn, size, np.float32)
    for k in INT_KEYS:
        assert got[k].dtype == np.int32
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in FLOAT_KEYS:
        rtol, r = rtol_from(f32[k], want[k]), ratio(got[k], want[k])
        print('%s %s: kernel %.1f eps32, float32 restatement %.1f eps32, bar %.1f eps32' % (name, k, r / EPS32, ratio(f32[k], want[k]) / EPS32, rtol / EPS32))
        assert r <= rtol, (k, r, rtol)
    assert (got['label'] > 0).any() and (got['label'] == 0).any() and (got['label'] < 0).any()


def _edge(train=True, size='pair', prev=True):
    c = cr.edge_case()
    return c, _refine(c, cr.EDGE_THRESH, cr.EDGE_STD, cr.EDGE_STD, c['pair'] if size == 'pair' else c['hw'], train=train, prev=prev)


@pytest.mark.parametrize('size', ['pair', 'per_image'])
def test_refine_edges_in_exact_arithmetic(size):
    c, got = _edge(size=size)
    e = c['expect']
    want = cr.refine(c['rois'], c['box_out'], cr.LOC0, c['N'], cr.MEAN, cr.EDGE_STD, c['pair'], c['prev_label'], c['gt_boxes'], c['gt_labels'],
                     c['n_gt'], cr.EDGE_THRESH, cr.EDGE_STD, dtype=np.float64)
    for k in got:
        assert np.isfinite(got[k]).all(), k                     # no NaN or inf anywhere: the zero-area gt, the +88 delta, the 1e30 padding rows
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], e[k], err_msg=k)
    np.testing.assert_array_equal(got['roi'], e['roi'])       # zero deltas: expf(0) = 1, every box exact
    np.testing.assert_array_equal(got['rois_xy5'][:, 0], np.repeat(np.arange(3), 4))
    np.testing.assert_array_equal(got['rois_xy5'][:, 1:], e['roi'][:, [1, 0, 3, 2]])
    assert got['label'][0] == 4 and got['gt_assign'][0] == 0          # IoU exactly 0.75 at thresh 0.75: foreground; equal IoUs take the first
    assert got['label'][1] == -1 and (got['roi'][1] == 100).all()      # pushed outside: zero area, ignored, finite
    assert (got['roi'][2] == (0, 0, 100, 100)).all() and got['label'][2] == 0      # +88: the full extent
    assert (got['label'][[4, 6]] == 0).all() and (got['gt_assign'][4:8] == -1).all()      # the image without ground truth
    assert got['label'][8] == 0 and not got['gt_loc'][8].any()        # zero-area gt: background, zero loc
    pad = [5, 7, 9, 10, 11]
    assert not got['roi'][pad].any() and not got['gt_loc'][pad].any() and not got['rois_xy5'][pad, 1:].any()
    assert (got['label'][pad] == -1).all() and (got['gt_assign'][pad] == -1).all() and (got['levels'][pad] == 0).all()
    fg = got['label'] > 0
    assert not got['gt_loc'][~fg].any() and got['gt_loc'][3].any()
    assert ratio(got['gt_loc'], want['gt_loc']) <= 16 * EPS32


def test_refine_inference_form_writes_the_training_forms_boxes():
    c, train = _edge()
    _, infer = _edge(train=False)
    assert sorted(infer) == ['levels', 'roi', 'rois_xy5']
    for k in infer:
        np.testing.assert_array_equal(infer[k], train[k], err_msg=k)
    # and on random rows, without previous labels: every row is live
    name, case, thr, sp, sn, size = _CASES[4]
    a = _refine(case, thr, sp, sn, size, train=False, prev=False)
    b = _refine(case, thr, sp, sn, size, train=True, prev=False)
    want = cr.refine(case['rois'], case['box_out'], cr.LOC0, case['N'], cr.MEAN, sp, size, dtype=np.float64)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a['levels'], want['levels'])


def test_refine_of_no_rows_and_bad_arguments():
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    z = ops.cascade_refine(torch.zeros((0, 4), device=DEV), torch.zeros((0, cr.LD), device=DEV), cr.LOC0, 2, cr.MEAN, cr.STDS[0], (10., 10.),
                           gt_boxes=torch.zeros((2, 3, 4), device=DEV), gt_labels=torch.zeros((2, 3), dtype=torch.int32, device=DEV),
                           n_gt=torch.zeros((2,), dtype=torch.int32, device=DEV), iou_thresh=0.6, std_next=cr.STDS[1])
    torch.cuda.synchronize()
    assert z['roi'].shape == (0, 4) and z['label'].shape == (0,)
    with pytest.raises(_hip.MrcnnHipError):           # more ground-truth boxes than the kernel stages in LDS
        ops.cascade_refine(torch.zeros((2, 4), device=DEV), torch.zeros((2, cr.LD), device=DEV), cr.LOC0, 1, cr.MEAN, cr.STDS[0], (10., 10.),
                           gt_boxes=torch.zeros((1, 257, 4), device=DEV), gt_labels=torch.zeros((1, 257), dtype=torch.int32, device=DEV),
                           n_gt=torch.zeros((1,), dtype=torch.int32, device=DEV), iou_thresh=0.6, std_next=cr.STDS[1])
    with pytest.raises(_hip.MrcnnHipError):           # the loc columns do not fit the row
        ops.cascade_refine(torch.zeros((2, 4), device=DEV), torch.zeros((2, cr.LD), device=DEV), cr.LD - 3, 1, cr.MEAN, cr.STDS[0], (10., 10.))
    with pytest.raises(ValueError):
        ops.cascade_refine(torch.zeros((2, 4), device=DEV), torch.zeros((2, cr.LD), device=DEV), cr.LOC0, 1, cr.MEAN, cr.STDS[0], (10., 10.),
                           gt_boxes=torch.zeros((1, 3, 4), device=DEV))


@pytest.mark.parametrize('n_class,K', [(81, 2), (81, 3), (2, 2), (2, 3)])
def test_cascade_prob_is_the_mean_of_the_stage_softmaxes(n_class, K):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(5 + n_class + K)
    R = 70
    outs = [(rs.standard_normal((R, cr.LD)) * 3).astype(np.float32) for _ in range(K)]
    outs[0][3, 1] = 1e4                       # no overflow: the maximum is subtracted first
    outs[K - 1][5, 0] = -1e4
    got = ops.cascade_prob([_t(o) for o in outs], n_class)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want, f32 = cr.prob_mean(outs, n_class, np.float64), cr.prob_mean(outs, n_class, np.float32)
    assert got.shape == (R, n_class) and np.isfinite(got).all()
    rtol, r = rtol_from(f32, want), ratio(got, want)
    print('prob n_class %d K %d: kernel %.1f eps32, bar %.1f eps32' % (n_class, K, r / EPS32, rtol / EPS32))
    assert r <= rtol
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 8 * EPS32
    with pytest.raises(ValueError):
        ops.cascade_prob([_t(outs[0])], n_class)


# ---- the model, the training chain and inference ----------------------------------------------------------------------------------------
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_keypoint_loss            # noqa: E402
from chainer_maskrcnn.model.head.fpn_roi_mask_head import roi_align_fpn_bwd            # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN            # noqa: E402
from chainer_maskrcnn.nn import core            # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay            # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch            # noqa: E402
import loss_reference as lr            # noqa: E402
from loss_judge import loss_close            # noqa: E402
from tests import step_harness            # noqa: E402

SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
IOUS = (0.5, 0.6, 0.7)
D64 = torch.float64


_build, _batch, _step, _check = functools.partial(step_harness.build, SHRINK), step_harness.batch, step_harness.step, step_harness.check
_predict_model = functools.partial(step_harness.predict_model, SHRINK)


def _cascade_names(m, k=None):
    return [n for n in m.ps.names() if n.startswith('head/cascade%s' % ('' if k is None else '%d/' % k))]


def test_defaults_are_untouched():
    """cascade_ious=None and a model built without the argument: the same offsets, parameters and flat gradient buffer, bit for bit."""
    res = []
    for kw in ({}, {'cascade_ious': None}):
        m, chain = _build(**kw)
        _step(chain, _batch())
        assert not m.cascade_heads and m.head.pool_grad_scale is None and chain.observation.keys() == {
            'rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss'}
        res.append((m.ps.params.clone(), m.ps.grads.clone(), dict(m.ps.offsets)))
    assert res[0][2] == res[1][2] and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0


def test_cascade_step_is_finite_and_bit_reproducible():
    m, chain = _build(cascade_ious=IOUS)
    chain.keep_outputs = True
    b = _batch()
    _step(chain, b)
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert all(np.isfinite(v) for v in obs.values()), obs
    for k in (2, 3):
        assert 'roi_loc_loss_s%d' % k in obs and 'roi_cls_loss_s%d' % k in obs
    rows = chain.outputs['losses'].cpu().numpy()
    assert rows.shape == (9, 2)
    total = np.float32(0)
    for v in rows[:, 0]:                    # mrcnn_loss_total_f32: the float32 sum of the rows' losses in row order
        total = np.float32(total + v)
    assert np.float32(obs['loss']) == total
    assert [obs[k] for k in ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'roi_loc_loss_s2', 'roi_cls_loss_s2',
                             'roi_loc_loss_s3', 'roi_cls_loss_s3')] == [float(v) for v in rows[:, 0]]
    g1 = m.ps.grads.clone()
    assert torch.isfinite(g1).all()
    names = _cascade_names(m)
    assert len(names) == 16
    for n in names:
        g = m.ps.g(n)
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, n
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)                      # no float atomics: the later stages accumulate in a fixed order


def test_cascade_wiring():
    m, chain = _build(cascade_ious=IOUS)
    chain.EARLY_RPN_BACKWARD = False
    chain.keep_outputs = True
    for h in m.box_stages:
        h.keep_pool_grad = True
    b = _batch()
    _step(chain, b)
    out, t, head = chain.outputs, chain.targets, m.head
    obs = {k: float(v) for k, v in chain.observation.items()}
    n, R = 2, t['gt_roi_label'].shape[0]
    nc, l0 = head.n_class, head.LOC0
    stage_in = [dict(roi=t['sample_roi'], rois_xy5=t['rois_xy5'], levels=t['sample_levels'], gt_loc=t['gt_roi_loc'], label=t['gt_roi_label'],
                     box=out['box'])] + out['cascade']
    assert len(stage_in) == 3
    # (a) each stage's two losses against the float64 references on the kept outputs, labels and targets
    for k, s in enumerate(stage_in, 1):
        box, lab, loc = s['box'].cpu().numpy(), s['label'].cpu().numpy(), s['gt_loc'].cpu().numpy()
        sfx = '' if k == 1 else '_s%d' % k
        loss_close(obs['roi_cls_loss' + sfx], lr.softmax_cross_entropy(box[:, :nc], lab)[0])
        loss_close(obs['roi_loc_loss' + sfx], lr.fast_rcnn_loc_loss(box[:, l0:l0 + 4], loc, lab, 1.0)[0])
        assert (lab > 0).any() and (lab == 0).any()
    # (b) stage k's inputs = a direct call of the refine kernel on stage k-1's kept tensors, bit for bit
    from chainer_maskrcnn._hip import ops
    stds = m.cascade_stds
    n_gt = ops.count_valid_labels(b['labels'].to(torch.int32).contiguous())
    for k in (2, 3):
        prev, cur = stage_in[k - 2], stage_in[k - 1]
        ref = ops.cascade_refine(prev['roi'], prev['box'], l0, n, m.loc_normalize_mean, stds[k - 2], (128., 160.), prev_label=prev['label'],
                                 gt_boxes=b['bboxes'].contiguous(), gt_labels=b['labels'].to(torch.int32).contiguous(), n_gt=n_gt,
                                 iou_thresh=IOUS[k - 1], std_next=stds[k - 1])
        for key, v in ref.items():
            assert torch.equal(v, cur[key]), (k, key)
    # (d) the pyramid gradient behind the heads: every stage's pooled gradient times float32(1 / K) through the ROIAlign backward, plus the mask's
    inv_k = torch.tensor(np.float32(1.0) / np.float32(3.0), device=DEV)
    scales = m.extractor.spatial_scales
    parts = []
    for h, s in zip(m.box_stages, stage_in):
        bufs = [torch.empty_like(f) for f in out['features']]
        roi_align_fpn_bwd((h.kept_pool_grad * inv_k).contiguous(), bufs, s['rois_xy5'], s['levels'], head.roi_size_box, scales, accumulate=False)
        parts.append(bufs)
    bufs = [torch.empty_like(f) for f in out['features']]
    roi_align_fpn_bwd(out['g_mask_pool'], bufs, chain.mask_inputs[0], chain.mask_inputs[1], head.roi_size_mask, scales, accumulate=False)
    parts.append(bufs)
    torch.cuda.synchronize()
    bad = []
    for l in range(len(out['features'])):
        p = [q[l].cpu() for q in parts]
        want64 = sum(x.to(D64) for x in p)
        want32 = ((p[3] + p[2]) + p[1]) + p[0]
        _check('pyramid gradient level %d' % l, out['g_feats_heads'][l], want64, want32, bad)
        assert l == 4 or float(want64.abs().max()) > 0          # (no RoI of 128 x 160 images reaches the coarsest level)
    assert not bad, bad
    # (c) stage k's parameter gradients = that stage's box_branch + backward_box alone on the kept inputs and loss gradient, bit for bit:
    # nothing scales them and nothing flows back through the refinement
    kept = {n_: m.ps.g(n_).clone() for n_ in _cascade_names(m)}
    for k in (2, 3):
        stage, s = m.cascade_heads[k - 2], stage_in[k - 1]
        m.ps.grads.zero_()
        again = stage.box_branch(out['features'], s['rois_xy5'], s['levels'], scales)
        assert torch.equal(again, s['box'])
        stage.backward_box(out['g_boxes'][k - 1], [torch.zeros_like(f) for f in out['features']], accumulate=True)
        core.join_side_stream(torch.device(DEV))
        torch.cuda.synchronize()
        for n_ in _cascade_names(m, k):
            assert torch.equal(m.ps.g(n_), kept[n_]), n_


def test_thirty_steps_reduce_the_loss():
    """The criterion and optimizer settings of tests/test_groupnorm_gpu.py::test_thirty_steps_reduce_the_loss with three box stages."""
    m, chain = _build(seed=11, cascade_ious=IOUS)
    opt = MomentumSGD(lr=0.01, momentum=0.9).setup(chain)
    opt.add_hook(WeightDecay(0.0005))
    b = _batch()
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss', 'roi_loc_loss_s2', 'roi_cls_loss_s2',
             'roi_loc_loss_s3', 'roi_cls_loss_s3')
    w0 = m.ps.p('head/cascade3/fc2/W').clone()
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
    assert last[3] < first[3] and last[9] < first[9], (first, last)
    assert torch.isfinite(m.ps.params).all()
    assert not torch.equal(w0, m.ps.p('head/cascade3/fc2/W'))


def test_graphed_step_with_cascade_replays_the_eager_step():
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build(cascade_ious=IOUS)
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
        res.append((m.ps.params.clone(), float(chain.observation['loss']), float(chain.observation['roi_cls_loss_s3'])))
    assert res[0][1:] == res[1][1:]
    assert torch.equal(res[0][0], res[1][0])


def test_giou_box_loss_with_cascade_is_finite_and_reproducible():
    m, chain = _build(cascade_ious=IOUS, chain_kw=dict(box_loss='giou', box_loss_weight=2.0))
    b = _batch()
    _step(chain, b)
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert all(np.isfinite(v) for v in obs.values()) and obs['roi_loc_loss_s3'] > 0, obs
    g1 = m.ps.grads.clone()
    assert torch.isfinite(g1).all() and all(float(m.ps.g(n).abs().max()) > 0 for n in _cascade_names(m))
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)


def test_keypoint_chain_with_two_stages_runs_one_step():
    K = 17
    m = MaskRCNN(n_fg_class=1, n_keypoints=K, head_arch='fpn_keypoint', device=DEV, seed=11, _test_shrink=SHRINK, cascade_ious=(0.5, 0.6))
    assert len(m.cascade_heads) == 1 and m.cascade_stds == ((0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1))
    chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_keypoint_loss, binary_mask=False)
    b = make_batch(5, 2, 128, 160, G=3, n_fg_class=1, n_keypoints=K)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [128, 160])
    b = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    chain(b['imgs'], b['bboxes'], b['labels'], b['keypoints'], 1.0).backward()
    torch.cuda.synchronize()
    assert 'roi_cls_loss_s2' in chain.observation and 'roi_cls_loss_s3' not in chain.observation
    assert all(np.isfinite(float(v)) for v in chain.observation.values())
    assert torch.isfinite(m.ps.grads).all()
    for n in _cascade_names(m):
        assert float(m.ps.g(n).abs().max()) > 0, n


def test_cascade_predict(tmp_path):
    from oracle import predict as opredict
    from chainer_maskrcnn.utils.chainer_npz import load_npz, save_npz
    m = _predict_model(5, cascade_ious=IOUS)
    rs = np.random.RandomState(0)
    a, b = (torch.from_numpy((rs.rand(3, h, w) * 255).astype(np.float32)) for h, w in ((120, 150), (100, 100)))
    alone = m.predict([a])
    alone_boxes = m.last_bboxes
    assert m.train is True and core.TRAIN is True
    assert alone[1][0].shape[0] > 0
    stages = [(r.cpu().numpy(), o.cpu().numpy()) for r, o in m.last_stages]
    assert len(stages) == 3 and m.last_rois is m.last_stages[-1][0]
    cls_bbox, prob = (t.cpu().numpy() for t in m.last_decoded)
    # the score: the mean of the kept stages' softmax
    outs = [o for _, o in stages]
    want, f32 = cr.prob_mean(outs, m.n_class, np.float64), cr.prob_mean(outs, m.n_class, np.float32)
    assert ratio(prob, want) <= rtol_from(f32, want)
    # the boxes: the last stage's deltas on its input boxes with its std (the bar of tests/test_predict_gpu.py for detect_decode)
    rois3, out3 = stages[-1]
    scale = m.prepare_size(120, 150)[1] / 150
    l0 = m.head.LOC0
    wb, _ = opredict.decode(rois3, out3[:, l0:l0 + 4], out3[:, :m.n_class], scale, (120, 150), m.n_class, std=m.cascade_stds[-1])
    np.testing.assert_allclose(cls_bbox, wb, rtol=1e-5, atol=1e-3)
    # stage k's input boxes are stage k-1's refined ones, in the prepared image's frame
    frame = tuple(float(v) for v in m.prepare_size(120, 150))
    for k in (1, 2):
        ref = cr.refine(stages[k - 1][0], stages[k - 1][1], l0, 1, m.loc_normalize_mean, m.cascade_stds[k - 1], frame, dtype=np.float64)
        f32r = cr.refine(stages[k - 1][0], stages[k - 1][1], l0, 1, m.loc_normalize_mean, m.cascade_stds[k - 1], frame, dtype=np.float32)
        assert ratio(stages[k][0], ref['roi']) <= rtol_from(f32r['roi'], ref['roi'])
    # an image's result does not depend on its batch neighbours
    both = m.predict([b, a])
    for k in range(3):
        assert torch.equal(alone[k][0], both[k][1])
    assert torch.equal(alone_boxes[0], m.last_bboxes[1])
    # the npz round trip
    path = str(tmp_path / 'cascade.npz')
    save_npz(path, m)
    fresh = _predict_model(6, cascade_ious=IOUS)
    assert not torch.equal(fresh.ps.params, m.ps.params)
    load_npz(path, fresh, strict=True)
    assert torch.equal(fresh.ps.params, m.ps.params)
    again = fresh.predict([a])
    for k in range(3):
        assert torch.equal(alone[k][0], again[k][0])
    assert torch.equal(alone_boxes[0], fresh.last_bboxes[0])
    # a plain model's file: stage 1, backbone and RPN are filled, the later stages keep their initialisation; strict refuses it
    plain = _predict_model(8)
    ppath = str(tmp_path / 'plain.npz')
    save_npz(ppath, plain)
    other = _predict_model(9, cascade_ious=IOUS)
    init = {n: other.ps.p(n).clone() for n in _cascade_names(other)}
    load_npz(ppath, other, strict=False)
    for n in plain.ps.names():
        assert torch.equal(other.ps.p(n), plain.ps.p(n)), n
    for n, v in init.items():
        assert torch.equal(other.ps.p(n), v), n
    with pytest.raises(KeyError):
        load_npz(ppath, other, strict=True)
    # Soft-NMS, voting and the cap run on top of the cascade's boxes and scores
    m.use_soft_nms('linear')
    m.use_box_voting(0.8)
    m.use_max_detections(5)
    post = m.predict([a])
    assert 0 < post[1][0].shape[0] <= 5 and torch.isfinite(m.last_bboxes[0]).all() and torch.isfinite(post[2][0]).all()
    with pytest.raises(ValueError):
        m.use_test_augmentation([160, 200])
