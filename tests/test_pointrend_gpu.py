"""PointRend on the GPU (csrc/pointrend.hip, PointHead, the training chain and inference) against
tests/pointrend_reference.py: every sampling kernel equals the float32 restatement bit for bit and the float64 one within a derived bound,
the selections equal the reference's exactly, the loss is judged as tests/loss_judge.py does."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointrend_reference as pr            # noqa: E402
from loss_judge import EPS32, loss_close, ratio, rtol_from            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
I32 = torch.int32
F32, F64 = np.float32, np.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(a, fill=7.0, extra=4096):
    """a copy of ``a`` on the device as a view of a larger buffer whose tail holds ``fill``."""
    buf = torch.full((a.size + extra,), fill, device=DEV)
    view = buf[:a.size].view(a.shape)
    view.copy_(_t(a))
    return buf, view


def _coord_slack(rois, scale):
    """delta: how far a frame coordinate in map units can move by float32 rounding.  X = fl(x1 + fl(u fl(x2 - x1))) carries three
    roundings of quantities no larger than M = max(|x1|, |x2|, |x2 - x1|) (u < 1), the scale is a power of two, the subtraction of 0.5 one
    more: |X32 - X64| scale <= 4 (eps32 / 2) 2 M scale = 4 eps32 M scale."""
    r = np.abs(rois[:, 1:].astype(F64))
    M = max(float(r.max()), float(np.abs(rois[:, 3] - rois[:, 1]).max()), float(np.abs(rois[:, 4] - rois[:, 2]).max()), 1.0)
    return 4 * EPS32 * M * scale


# ---- point_features_fwd / point_features_bwd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,C,P', [(9, 13, 32, 7), (16, 24, 256, 196), (9, 13, 256, 196), (16, 24, 32, 7)])
def test_features_forward_and_backward(H, W, C, P):
    """Bit equality with the float32 restatement, which rounds as the kernel does.  Against float64: a weight is a product of two
    differences of exactly representable fractions - (1 - l) rounds once, the product once -, the tap product rounds once and the three
    additions once each, so the four-term sum is within 6 (eps32 / 2) sum |w x| <= 4 eps32 sum |w x| of the sum with exact weights at the
    float32 coordinates.  The coordinates themselves differ from float64's by at most delta (see _coord_slack) per axis, and bilinear
    interpolation of the zero-extended map moves by at most 2 max|x| per unit of either coordinate (also across a change of floor: it is
    continuous): |got - want64| <= 4 eps32 sum |w x| + 4 delta max |x|.  The backward is the transpose: a cell's sum of n tap products
    and the prior value takes n additions, each product three roundings, so it is within (n + 3) eps32 (sum |w g| + |prior|) of the sum with
    exact weights; a weight moves by at most delta per axis, 2 delta in all, also where the floor changes and the tap lands on the
    neighbouring cell: + 2 delta times the sum of |g| over the taps that land on the cell in either arithmetic."""
    from chainer_maskrcnn._hip import ops
    c = pr.feature_case(H, W, C, P)
    scale = 0.25
    args = (_t(c['coords']), _t(c['rois']), _t(c['fmap']), scale, _t(c['coarse']), c['n_fg'], c['cin_p'])
    got_t = ops.point_features_fwd(*args)
    torch.cuda.synchronize()
    got = got_t.cpu().numpy().reshape(5, P, -1)
    w32 = pr.features_fwd(c['coords'], c['rois'], c['fmap'], scale, c['coarse'], c['n_fg'], c['cin_p'], F32)
    w64 = pr.features_fwd(c['coords'], c['rois'], c['fmap'], scale, c['coarse'], c['n_fg'], c['cin_p'], F64)
    np.testing.assert_array_equal(got, w32)
    assert got.shape == (5, P, c['cin_p']) and not got[..., C + c['n_fg']:].any() and got[..., :C].any() and got[..., C:C + c['n_fg']].any()
    sabs = pr.features_fwd(c['coords'], c['rois'], np.abs(c['fmap']), scale, np.abs(c['coarse']), c['n_fg'], c['cin_p'], F64)
    delta_f, delta_c = _coord_slack(c['rois'], scale), 2 * EPS32 * c['coarse'].shape[1]
    bound = 4 * EPS32 * sabs
    bound[..., :C] += 4 * delta_f * float(np.abs(c['fmap']).max())
    bound[..., C:] += 4 * delta_c * float(np.abs(c['coarse']).max())
    err = np.abs(got.astype(F64) - w64)
    print('fwd %dx%d C %d P %d: worst err / bound %.3f' % (H, W, C, P, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert torch.equal(ops.point_features_fwd(*args), got_t)                # twice, identical bits
    # the row partly outside the map has points whose taps are all outside: zeros, and the point (0, 0) of row 0 is one of them
    assert not got[0, 0, :C].any()
    empty = ops.point_features_fwd(torch.zeros((0, P, 2), device=DEV), torch.zeros((0, 5), device=DEV), _t(c['fmap']), scale,
                                   torch.zeros((0,) + c['coarse'].shape[1:], device=DEV), c['n_fg'], c['cin_p'])
    assert empty.shape == (0, 1, P, c['cin_p'])
    # backward, with and without a prior gradient in the map; the guard region behind the map stays untouched
    for prior in (np.zeros_like(c['g_map']), c['g_map']):
        outs = []
        for _ in range(2):
            buf, view = _guarded(prior)
            out = ops.point_features_bwd(_t(c['g_in']).view(5, 1, P, -1), _t(c['coords']), _t(c['rois']), scale, view)
            torch.cuda.synchronize()
            assert out.data_ptr() == view.data_ptr() and bool((buf[prior.size:] == 7.0).all())
            outs.append(view.cpu().numpy())
        np.testing.assert_array_equal(outs[0], outs[1])                     # twice, identical bits
        b32 = pr.features_bwd(c['g_in'], c['coords'], c['rois'], scale, prior, F32)
        b64 = pr.features_bwd(c['g_in'], c['coords'], c['rois'], scale, prior, F64)
        np.testing.assert_array_equal(outs[0], b32)
        babs = pr.features_bwd(np.abs(c['g_in']), c['coords'], c['rois'], scale, np.abs(prior), F64)
        ones = np.ones_like(c['g_in'])
        n_taps = pr.features_bwd(ones, c['coords'], c['rois'], scale, np.zeros_like(prior), F64, unit_weights=True)
        g_taps = sum(pr.features_bwd(np.abs(c['g_in']), c['coords'], c['rois'], scale, np.zeros_like(prior), dt, unit_weights=True).astype(F64)
                     for dt in (F32, F64))
        bound = (n_taps + 3) * EPS32 * babs + 2 * delta_f * g_taps
        err = np.abs(outs[0].astype(F64) - b64)
        print('bwd prior %s: worst err / bound %.3f, %d cells touched' % (bool(prior.any()), float((err / np.maximum(bound, 1e-300)).max()),
                                                                          int((n_taps[..., 0] > 0).sum())))
        assert (err <= bound).all() and (outs[0] != prior).any()
        assert np.array_equal(outs[0][n_taps == 0], prior[n_taps == 0])     # cells no tap lands on keep their bits


# ---- point_train_coords -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S0,n_fg,P,k', [(6, 3, 8, 3), (28, 80, 196, 3), (28, 80, 8, 3), (6, 3, 196, 3)])
def test_train_coords_select_the_reference_points(S0, n_fg, P, k):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(S0 + n_fg + P)
    rows, Cp, n_cand, n_imp = 6, pr.pad32(n_fg), k * P, int(np.floor(0.75 * P))
    coarse = (rs.standard_normal((rows, S0, S0, Cp)) * 2).astype(F32)
    coarse[2] = 0.0                                         # equal uncertainties everywhere: the tie rule alone orders the row
    coarse[3] = np.round(coarse[3])                         # many exact ties among a few values
    label = np.array([1, n_fg, 1, 2, 0, -1], np.int32)      # the first and the last class channel; a background and a padding row
    n_keys = ops.point_n_keys(P, n_cand, n_imp)
    keys = rs.randint(0, 2 ** 32, (rows, n_keys), dtype=np.uint64).astype(np.uint32).view(np.int32)
    keys[1, 4:6] = keys[1, 0:2]                             # two candidates at one position
    got = ops.point_train_coords(_t(keys), _t(coarse), _t(label), n_fg, P, n_cand, n_imp)
    torch.cuda.synchronize()
    want, picked = pr.train_coords(keys, coarse, label, n_fg, P, n_cand, n_imp)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert got.shape == (rows, P, 2) and float(got.min()) >= 0 and float(got.max()) < 1
    for r in (2, 4, 5):                                     # all ties / no channel: the first n_imp candidates in index order
        np.testing.assert_array_equal(picked[r], np.arange(n_imp))
    assert not np.array_equal(picked[0], np.arange(n_imp)) and len(set(picked[0])) == n_imp
    # the remainder are the keys behind the candidates'
    np.testing.assert_array_equal(got.cpu().numpy()[:, n_imp:].reshape(rows, -1), pr.key_unit(keys)[:, 2 * n_cand:])
    assert torch.equal(ops.point_train_coords(_t(keys), _t(coarse), _t(label), n_fg, P, n_cand, n_imp), got)
    base0 = ops.point_train_coords(_t(keys), _t(coarse), _t((label - 1).astype(np.int32)), n_fg, P, n_cand, n_imp, label_base=0)
    assert torch.equal(base0, got)
    assert ops.point_train_coords(torch.zeros((0, n_keys), dtype=I32, device=DEV), torch.zeros((0, S0, S0, Cp), device=DEV),
                                  torch.zeros((0,), dtype=I32, device=DEV), n_fg, P, n_cand, n_imp).shape == (0, P, 2)


# ---- point_target -------------------------------------------------------------------------------------------------------------------------
def test_target_samples_the_assigned_mask():
    """The target is a four-term weighted sum of zeros and ones: within 4 eps32 of the sum with exact weights, plus the move of the
    coordinates (delta per axis, no scale) times the slope 2 of a 0/1 map - the bound of test_features_forward_and_backward with max|x| = 1."""
    from chainer_maskrcnn._hip import ops
    c = pr.target_case()

    def run(case):
        o = ops.point_target(_t(case['masks']), _t(case['n_gt']), _t(case['rois']), _t(case['gt_assign']), _t(case['label']), _t(case['n_pos']),
                             case['n_sample'], case['rows'], _t(case['coords']))
        torch.cuda.synchronize()
        return o.cpu().numpy()
    got = run(c)
    a = (c['masks'], c['n_gt'], c['rois'], c['gt_assign'], c['label'], c['n_pos'], c['n_sample'], c['rows'], c['coords'])
    w32, w64 = pr.target(*a, F32), pr.target(*a, F64)
    np.testing.assert_array_equal(got, w32)
    live = pr.live_rows(c['n_gt'], c['gt_assign'], c['label'], c['n_pos'], c['n_sample'], c['rows'], 3)
    assert live.tolist() == [True, True, False, False, False, False, True, False, True, True, False, False]
    assert (got[~live] == -1).all() and (got[live] >= 0).all() and (got[live] <= 1).all()
    assert ((got[live] > 0) & (got[live] < 1)).any() and (got[live] == 0).any() and (got[live] == 1).any()
    assert (np.abs(got.astype(F64) - w64) <= 4 * EPS32 + 4 * _coord_slack(c['rois'], 1.0)).all()
    assert got[0, 0] == np.float32(0.25) * (c['masks'][0, 0, 0, 0] != 0)        # the image's corner: one tap inside, weight 1/4
    clean = dict(c, masks=c['masks'].copy())
    clean['masks'][0, 2] = 0                                                    # the junk of the unused slot does not matter
    np.testing.assert_array_equal(run(clean), got)


# ---- point_bce ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,n_fg,P,weight', [(1, 3, 7, 1.0), (16, 80, 49, 2.5), (1500, 80, 7, 0.3)])
def test_bce_against_float64(rows, n_fg, P, weight):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(rows + n_fg)
    ld = pr.pad32(n_fg)
    pred = (rs.standard_normal((rows, 1, P, ld)) * 3).astype(F32)
    tgt = rs.rand(rows, P).astype(F32)
    tgt[rs.rand(rows, P) < 0.3] = 0.0
    tgt[rs.rand(rows, P) < 0.3] = 1.0
    label = rs.randint(1, n_fg + 1, rows).astype(np.int32)
    if rows > 1:
        tgt[1::5] = -1.0                                    # rows that are not live
        label[-1] = n_fg                                    # the last logical channel
        label[2] = 0                                        # a background row that carries targets: skipped
    out, gx = ops.point_bce(_t(pred), _t(tgt), _t(label), n_fg, weight=weight)
    torch.cuda.synchronize()
    out, gx = out.cpu().numpy(), gx.cpu().numpy().reshape(rows, P, ld)
    w_loss, w_count, w_gx = pr.bce(pred, tgt, label, n_fg, weight, dt=F64)
    f_loss, _, f_gx = pr.bce(pred, tgt, label, n_fg, weight, dt=F32)
    extra = (w_gx != 0) * (weight / w_count)                # where the target was subtracted from the sigmoid
    rg = rtol_from(f_gx, w_gx, extra)
    print('bce rows %d: loss %.3e rel, gradient %.1f eps32 (bar %.1f)' % (rows, abs(float(out[0]) - w_loss) / w_loss, ratio(gx, w_gx, extra) / EPS32,
                                                                         rg / EPS32))
    assert out[1] == w_count and w_count == int(((tgt >= 0) & (label > 0)[:, None]).sum())
    loss_close(out[0], w_loss)
    assert ratio(gx, w_gx, extra) <= rg
    assert not gx[w_gx == 0].any() and gx[w_gx != 0].all()
    out2, none = ops.point_bce(_t(pred), _t(tgt), _t(label), n_fg, weight=weight, want_grad=False)
    assert none is None and torch.equal(out2.cpu(), torch.from_numpy(out))


def test_bce_without_any_live_row_is_zero():
    from chainer_maskrcnn._hip import ops
    pred = torch.randn((9, 1, 7, 32), device=DEV)
    label = torch.randint(1, 4, (9,), dtype=I32, device=DEV)
    gx = torch.full((9, 1, 7, 32), 3.0, device=DEV)
    out, g = ops.point_bce(pred, torch.full((9, 7), -1.0, device=DEV), label, 3, gx=gx)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 1.0] and g is gx and not bool(gx.any())
    out, g = ops.point_bce(torch.zeros((0, 1, 7, 32), device=DEV), torch.zeros((0, 7), device=DEV), torch.zeros((0,), dtype=I32, device=DEV), 3)
    assert out.cpu().tolist() == [0.0, 1.0] and g.shape == (0, 1, 7, 32)


# ---- point_subdivide / point_scatter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,N,ld', [(4, 5, 32), (4, 100, 32), (56, 784, 1), (28, 784, 96)])
def test_subdivide_and_scatter(S, N, ld):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(S + N)
    D, n_fg = 3, min(ld, 80)
    logits = (rs.standard_normal((D, S, S, ld)) * 2).astype(F32)
    logits[1] = np.round(logits[1] * 2) / 2                 # a grid of a few values and zeros: ties, the upsample included
    label = np.array([0, n_fg - 1, min(1, n_fg - 1)], np.int32)
    up, index, coords = ops.point_subdivide(_t(logits), _t(label) if ld > 1 else None, n_fg, N)
    torch.cuda.synchronize()
    w_up, w_index, w_coords = pr.subdivide(logits[np.arange(D), :, :, label], N)
    n_sel = min(N, 4 * S * S)
    assert up.shape == (D, 2 * S, 2 * S) and index.shape == (D, n_sel) and coords.shape == (D, n_sel, 2)
    np.testing.assert_array_equal(up.cpu().numpy(), w_up)
    np.testing.assert_array_equal(index.cpu().numpy(), w_index)
    np.testing.assert_array_equal(coords.cpu().numpy(), w_coords)
    chosen = logits[np.arange(D), :, :, label]
    up64 = np.stack([pr.upsample2x(g, F64) for g in chosen])
    assert (np.abs(w_up.astype(F64) - up64) <= 4 * EPS32 * np.stack([pr.upsample2x(np.abs(g), F64) for g in chosen])).all()   # the weights are exact
    if N >= 4 * S * S:
        np.testing.assert_array_equal(w_index, np.arange(4 * S * S)[None].repeat(D, 0))
    pred = rs.standard_normal((D, 1, n_sel, 32)).astype(F32)
    lab2 = np.array([0, 2, 31], np.int32)
    buf, view = _guarded(w_up)
    ops.point_scatter(_t(pred), _t(lab2), index, 32, view)
    torch.cuda.synchronize()
    want = w_up.reshape(D, -1).copy()
    for d in range(D):
        want[d, w_index[d]] = pred[d, 0, :, lab2[d]]
    np.testing.assert_array_equal(view.cpu().numpy().reshape(D, -1), want)                  # cells outside the selection keep the upsampled value
    assert bool((buf[w_up.size:] == 7.0).all())
    e = ops.point_subdivide(torch.zeros((0, S, S, ld), device=DEV), None, 1, N)
    assert e[0].shape == (0, 2 * S, 2 * S) and e[1].shape == (0, n_sel)
    ops.point_scatter(torch.zeros((0, 1, n_sel, 32), device=DEV), torch.zeros((0,), dtype=I32, device=DEV), e[1], 32, e[0])


def test_ops_refuse_host_tensors():
    from chainer_maskrcnn._hip import ops
    with pytest.raises(Exception):
        ops.point_subdivide(torch.zeros((1, 4, 4, 32)), None, 1, 5)
    with pytest.raises(Exception):
        ops.point_features_bwd(torch.zeros((1, 1, 2, 32)), torch.zeros((1, 2, 2)), torch.zeros((1, 5)), 0.25, torch.zeros((1, 4, 4, 32)))


# ---- the model, the training chain and inference ------------------------------------------------------------------------------------------
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain            # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN            # noqa: E402
from chainer_maskrcnn.nn import core            # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay            # noqa: E402
from tests import step_harness            # noqa: E402

SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
SIX = {'rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss'}
POINT = dict(point_rend=True, point_train_points=49)           # a quarter of the default points: the kernels' tests cover 196


_build, _batch, _rel = functools.partial(step_harness.build, SHRINK), step_harness.batch, step_harness.check
_forward, _step = step_harness.forward, step_harness.step
_predict_model = functools.partial(step_harness.predict_model, SHRINK)


def _point_keys(chain, m, rows_total, seed=3):
    st = m.point_rend
    from chainer_maskrcnn._hip import ops
    n_keys = ops.point_n_keys(st['train_points'], st['n_candidates'], st['n_important'])
    rs = np.random.RandomState(seed)
    return _t(rs.randint(0, 2 ** 32, (rows_total, n_keys), dtype=np.uint64).astype(np.uint32).view(np.int32))


def _own(m):
    return [n for n in m.ps.names() if n.startswith('head/point/')]


@pytest.mark.parametrize('mask_rows', ['all', 'positives'])
def test_wiring(mask_rows):
    from chainer_maskrcnn._hip import ops
    m, chain = _build(mask_rows=mask_rows, chain_kw=dict(point_loss_weight=1.5), **POINT)
    chain.EARLY_RPN_BACKWARD = False
    chain.keep_outputs = True
    b = _batch()
    S = chain.proposal_target_creator.n_sample
    rows = S if mask_rows == 'all' else chain.proposal_target_creator.pos_cap
    chain.point_keys = _point_keys(chain, m, 2 * rows)
    _step(chain, b)
    out, t, ph, st = chain.outputs, chain.targets, m.point_head, m.point_rend
    pt = out['point']
    obs = {k: float(v) for k, v in chain.observation.items()}
    assert obs.keys() == SIX | {'point_loss'} and all(np.isfinite(v) for v in obs.values())
    assert t['mask_rows'] == rows
    P, C, n_fg = st['train_points'], m.head.channels, 80
    m_rois, m_label = chain.mask_inputs[0].contiguous(), chain.mask_inputs[2].contiguous()
    n_gt = ops.count_valid_labels(b['labels'].to(I32).contiguous())
    label = m_label.cpu().numpy()
    rois = m_rois.cpu().numpy()
    coords = pt['coords'].cpu().numpy()
    # the kept tensors are what the kernels give on the kept inputs, and what the reference gives
    w_coords, _ = pr.train_coords(chain.point_keys.cpu().numpy(), out['mask'].cpu().numpy(), label, n_fg, P, st['n_candidates'], st['n_important'])
    np.testing.assert_array_equal(coords, w_coords)
    scale0 = m.extractor.spatial_scales[0]
    w_in = pr.features_fwd(coords, rois, out['features'][0].cpu().numpy(), scale0, out['mask'].cpu().numpy(), n_fg, ph.cin_p, F32)
    np.testing.assert_array_equal(pt['input'].cpu().numpy().reshape(w_in.shape), w_in)
    w_tgt = pr.target(b['masks'].cpu().numpy(), n_gt.cpu().numpy(), rois, t['gt_assign'].cpu().numpy(), label, t['n_pos'].cpu().numpy(), S, rows,
                      coords, F32)
    np.testing.assert_array_equal(pt['target'].cpu().numpy(), w_tgt)
    live = w_tgt[:, 0] >= 0
    assert live.any() and not live.all() and ((w_tgt > 0) & (w_tgt < 1)).any()
    # (a) the loss and the head's parameter gradients against float64, evaluated on the kept input and target
    params = {n: m.ps.p(n).cpu().numpy() for n in _own(m)}
    x0 = w_in.reshape(-1, ph.cin_p)
    bad, grads = [], {}
    for dt in (F64, F32):
        pred, tape = pr.head_forward(params, x0, C, n_fg, dt)
        loss, count, gx = pr.bce(pred.reshape(len(label), P, -1), w_tgt, label, n_fg, 1.5, dt=dt)
        grads[dt] = (pred, loss, count, gx) + pr.head_backward(tape, gx, C, dt)
    pred64, loss64, count64, gx64, pg64, gin64 = grads[F64]
    _rel('point head forward', pt['pred'].cpu().numpy().reshape(pred64.shape), pred64, grads[F32][0], bad)
    rows_l = out['losses'].cpu().numpy()
    assert rows_l.shape == (6, 2) and rows_l[5, 1] == count64 == live.sum() * P and float(rows_l[5, 0]) == obs['point_loss']
    print('point_loss %.6f, float64 on the kept input %.6f' % (obs['point_loss'], loss64))
    assert abs(obs['point_loss'] - loss64) <= 1e-3 * loss64                         # through the float64 head: the GEMMs' bar, not the loss kernel's
    w_loss, _, w_gx = pr.bce(pt['pred'].cpu().numpy(), w_tgt, label, n_fg, 1.5, dt=F64)                      # the loss kernel alone: its own bar
    loss_close(obs['point_loss'], w_loss)
    total = np.float32(0)
    for v in rows_l[:, 0]:
        total = np.float32(total + v)
    assert np.float32(obs['loss']) == total
    for n in _own(m):
        k = n[len('head/point/'):]
        _rel(n, m.ps.g(n).cpu().numpy(), pg64[k], grads[F32][4][k], bad)
        assert float(m.ps.g(n).abs().max()) > 0, n
    _rel('fine input gradient', pt['g_in'].cpu().numpy().reshape(gin64.shape)[:, :C], gin64[:, :C], grads[F32][5][:, :C], bad)
    assert not bad, bad
    assert not pt['g_pred'].cpu().numpy().reshape(len(label), P, -1)[~live].any()           # rows that are not live: no gradient
    # (c) the stride-4 level's gradient behind the heads = what the ROIAlign backward passes left + the fine gradient, in the documented order
    before, after = out['g_feats0_heads'].cpu().numpy(), out['g_feats0_point'].cpu().numpy()
    np.testing.assert_array_equal(after, pr.features_bwd(pt['g_in'].cpu().numpy(), coords, rois, scale0, before, F32))
    assert (after != before).any()
    # (b) against the same step without the head: the mask logits' gradient, every loss and every other head / RPN gradient, bit for bit
    kept = {n: m.ps.g(n).clone() for n in m.ps.names()}
    m0, chain0 = _build(mask_rows=mask_rows)
    chain0.EARLY_RPN_BACKWARD = False
    assert m0.ps.names() == m.ps.names()[:len(m0.ps.names())] and torch.equal(m0.ps.params, m.ps.params[:m0.ps.size])
    loss0 = _forward(chain0, b)
    g_mask0 = chain0.pending.g_mask.clone()
    loss0.backward()
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    assert torch.equal(out['g_mask'], g_mask0) and float(g_mask0.abs().max()) > 0
    for k in SIX - {'loss'}:
        assert obs[k] == float(chain0.observation[k]), k
    for n in m0.ps.names():
        if n.startswith('head/') or n.startswith('rpn/'):
            assert torch.equal(kept[n], m0.ps.g(n)), n


def test_step_is_bit_reproducible_and_upstream_scales_the_seed():
    m, chain = _build(**POINT)
    b = _batch()
    chain.point_keys = _point_keys(chain, m, 2 * chain.proposal_target_creator.n_sample)
    _step(chain, b)
    g1 = m.ps.grads.clone()
    own1 = {n: m.ps.g(n).clone() for n in _own(m)}
    assert torch.isfinite(g1).all() and len(own1) == 8
    _step(chain, b)
    assert torch.equal(g1, m.ps.grads)
    _forward(chain, b)
    chain.backward(upstream=torch.tensor(2.0, device=DEV))
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    for n in _own(m):                  # a power of two scales every product and sum exactly
        assert torch.equal(m.ps.g(n), own1[n] * 2) and float(own1[n].abs().max()) > 0, n
    # the chain's own keys: another draw every step, no override needed
    chain.point_keys = None
    _step(chain, b)
    c1 = chain.key_streams['point_rend'].state.clone()
    _step(chain, b)
    assert not torch.equal(c1, chain.key_streams['point_rend'].state) and torch.isfinite(m.ps.grads).all()
    # the trainer state carries the seed state of the point keys: a resumed run draws the keys the original run would have drawn
    opt = MomentumSGD(lr=0.01, momentum=0.9).setup(chain)
    state = opt.state_dict()
    assert torch.equal(state['samplers']['point_rend']['state'], chain.key_streams['point_rend'].state.cpu())
    chain.keep_outputs = True
    _step(chain, b)
    m2, chain2 = _build(**POINT)
    opt2 = MomentumSGD(lr=0.01, momentum=0.9).setup(chain2)
    opt2.load_state_dict(state)
    assert torch.equal(chain2.key_streams['point_rend'].state, state['samplers']['point_rend']['state'].to(DEV))
    chain2.keep_outputs = True
    _step(chain2, b)
    assert torch.equal(chain2.outputs['point']['coords'], chain.outputs['point']['coords'])
    plain_state = MomentumSGD(lr=0.01).setup(_build()[1]).state_dict()
    assert 'point_rend' not in plain_state['samplers']
    creators = {'proposal_target_creator', 'anchor_target_creator'}         # the file format: these names, these two fields
    for saved, names in ((state, creators | {'point_rend'}), (plain_state, creators)):
        assert set(saved['samplers']) == names and all(set(entry) == {'seed', 'state'} for entry in saved['samplers'].values())


def test_thirty_steps_reduce_the_loss():
    """The criterion and optimizer settings of tests/test_maskiou_gpu.py::test_thirty_steps_reduce_the_loss with the point head; nothing is
    asserted about the trend of point_loss itself (its first and last values are printed, and recorded in DESIGN.md section 3.24)."""
    m, chain = _build(seed=11, **POINT)
    opt = MomentumSGD(lr=0.01, momentum=0.9).setup(chain)
    opt.add_hook(WeightDecay(0.0005))
    b = _batch()
    names = ('rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss', 'loss', 'point_loss')
    w0 = m.ps.p('head/point/fc2/W').clone()
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
    print('point_loss first step %.6f, last step %.6f' % (h[0, 6], h[-1, 6]))
    assert last[5] <= 0.5 * first[5], (first, last)
    assert torch.isfinite(m.ps.params).all()
    assert not torch.equal(w0, m.ps.p('head/point/fc2/W'))


def test_graphed_step_replays_the_eager_step():
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build(**POINT)
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
        res.append((m.ps.params.clone(), float(chain.observation['loss']), float(chain.observation['point_loss']), chain.key_streams['point_rend'].state.clone()))
    assert res[0][1:3] == res[1][1:3]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][3], res[1][3])          # the point keys advance alike under replay


def test_predict_refines_the_masks():
    from chainer_maskrcnn._hip import ops
    m = _predict_model(5, point_rend=True, subdivision_points=300)
    m.ps.p('head/point/predictor/W').mul_(300.0)    # freshly initialised predictions are near 0: make them matter
    plain = _predict_model(6)
    plain.ps.params.copy_(m.ps.params[:plain.ps.size])
    for model in (m, plain):                        # a dozen detections keep the NumPy restatement of the subdivision quick
        model.use_max_detections(12)
    rs = np.random.RandomState(0)
    img = torch.from_numpy((rs.rand(3, 120, 150) * 255).astype(np.float32))
    # (e1) without refinement: the masks of the same weights without the head, bit for bit
    m.point_rend_refine = False
    coarse_masks, labels0, scores0 = m.predict([img])
    assert m.last_point_grid is None and m.last_point_coarse is not None
    p_masks, p_labels, p_scores = plain.predict([img])
    assert torch.equal(coarse_masks[0], p_masks[0]) and torch.equal(labels0[0], p_labels[0]) and torch.equal(scores0[0], p_scores[0])
    m.point_rend_refine = True
    masks, labels, scores = m.predict([img])
    assert m.train is True and core.TRAIN is True
    D = labels[0].shape[0]
    assert D > 0 and torch.equal(labels[0], labels0[0]) and torch.equal(scores[0], scores0[0]) and masks[0].shape == coarse_masks[0].shape
    grid = m.last_point_grid
    assert grid.shape == (D, 112, 112)
    # (e2) the grid = the reference subdivision of the kept coarse logits and features (the point head's GEMMs are the model's own)
    coarse = m.last_point_coarse.cpu().numpy()
    lab = labels[0].to(I32).cpu().numpy()
    rois = m._xy5(m.last_bboxes[0], m.prepare_size(120, 150)[1] / 150).cpu().numpy()
    fmap = m.head.x[0].cpu().numpy()
    ph = m.point_head
    g = coarse[np.arange(D), :, :, lab]
    with m._inference_mode():
        for step in range(2):
            up, index, coords = pr.subdivide(g, 300)
            x_in = pr.features_fwd(coords, rois, fmap, m.extractor.spatial_scales[0], coarse, 80, ph.cin_p, F32)
            pred = ph.forward(_t(x_in).view(D, 1, -1, ph.cin_p)).cpu().numpy().reshape(D, index.shape[1], -1)
            flat = up.reshape(D, -1)
            for d in range(D):
                flat[d, index[d]] = pred[d, :, lab[d]]
            g = flat.reshape(up.shape)
    np.testing.assert_array_equal(grid.cpu().numpy(), g)
    assert (g != pr.subdivide(pr.subdivide(coarse[np.arange(D), :, :, lab], 1)[0], 1)[0]).any()                 # the head's predictions are in it
    # (e3) the pasted masks = mask_paste of that grid
    want = ops.mask_paste(grid.view(D, 112, 112, 1).contiguous(), torch.zeros((D,), dtype=I32, device=DEV), m.last_bboxes[0], (120, 150)).bool()
    assert torch.equal(masks[0], want) and not torch.equal(masks[0], coarse_masks[0])
    with pytest.raises(ValueError, match='point_rend'):
        m.use_test_augmentation([160, 200])


def test_empty_results_run_clean():
    """(f) no detection: nothing is refined and nothing is launched; an image without objects trains with a finite step."""
    m = _predict_model(5, point_rend=True)
    m.score_thresh = 2.0
    rs = np.random.RandomState(1)
    masks, labels, scores = m.predict([torch.from_numpy((rs.rand(3, 100, 100) * 255).astype(np.float32))])
    assert masks[0].shape == (0, 100, 100) and labels[0].shape == (0,) and m.last_point_grid is None and m.last_point_coarse is None
    m2, chain = _build(**POINT)
    b = _batch()
    b['labels'][1] = -1
    b['bboxes'][1] = 0
    b['masks'][1] = 0
    _step(chain, b)
    assert all(np.isfinite(float(v)) for v in chain.observation.values()) and torch.isfinite(m2.ps.grads).all()


def test_refusals_on_the_device():
    with pytest.raises(ValueError, match='point_rend'):
        MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', device=DEV, _test_shrink=SHRINK, point_rend=True)
    with pytest.raises(ValueError, match='mask_iou'):
        MaskRCNN(n_fg_class=5, device=DEV, _test_shrink=SHRINK, point_rend=True, mask_iou=True)
    m = MaskRCNN(n_fg_class=5, device=DEV, _test_shrink=SHRINK, point_rend=True)
    with pytest.raises(ValueError, match='mask_loss_fun'):
        FPNMaskRCNNTrainChain(m, mask_loss_fun=lambda *a: None)
