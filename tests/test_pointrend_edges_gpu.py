"""The PointRend kernels past five rows, one ballot, one lane trip and one grid pass (csrc/pointrend.hip, csrc/point_common.h;
DESIGN.md section 3.24), through ops.* against tests/pointrend_reference.py on the cases of tests/pointrend_edge_cases.py
(tests/test_pointrend_edge_cases_cpu.py holds every case to its path without a device).

Yardsticks, as in tests/test_pointrend_gpu.py: bit equality with the float32 restatement for the sampling kernels, the copies and the
selections (integers: equality); against float64 the bounds derived there - 4 eps32 sum |w x| + 4 delta max |x| forward, (n_taps + 3)
eps32 (sum |w g| + |prior|) + 2 delta g_taps backward -; tests/loss_judge.py for the loss; guard regions and untouched maps through
their uint32 view; every kernel twice with the same bits.

What the older file cannot see (rows = 5, C <= 256, patches a multiple of 4, one grid pass) and a wrong variant each test rejects:
  row ballot, ordered sum        `r0 < rows` of the `r0 += 64` loop - with one trip the rows from 64 on never add; `rmask &= rmask - 1` in
                                 ascending order and the point ballot's second trip - another order gives other bits on the piled cells
  channels                       `q += 64` of the load, add and store loops - a single trip leaves channels 256.. of C = 260 / 512 untouched;
                                 the LDS refusal at C = 516
  patch geometry                 `patch >= n_patches` - without it the idle waves of the last workgroup write past the map (the guard);
                                 `cy < ye && cx < xe` on the cropped edge patches; an image no tap lands on keeps a NaN payload
  boxes, indices                 fminf / fmaxf of the row filter (inverted boxes), the clamp to [-2, size], idx == img
  second grid pass               `pt += gridDim.x * (NT / 64)` of k_point_features_fwd
  coarse part                    the `c0 + k >= n_channels` zeros where the logical channels end inside a float4
  ranking                        the (bits of |value|, index) key: padding keys of the bitonic sort, zeros first, NaN last
  subdivision                    the tie rule (`e++ < need`), labels outside [0, n_channels), indices outside [0, cells)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointrend_edge_cases as cases            # noqa: E402
import pointrend_reference as pr            # noqa: E402
from loss_judge import EPS32, loss_close, ratio, rtol_from            # noqa: E402
from pointrend_edge_cases import F32, F64, SCALE            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
I32 = torch.int32
GUARD = 0x7fa5a5a5              # the bits behind every output: a NaN no kernel produces


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(a, extra=4096):
    """a copy of the float32 array ``a`` on the device as a view of a larger buffer whose tail holds GUARD."""
    buf = torch.full((a.size + extra,), GUARD, dtype=I32, device=DEV).view(torch.float32)
    view = buf[:a.size].view(a.shape)
    view.copy_(_t(a))
    return buf, view


def _guard_ok(buf, n):
    return bool((buf[n:].view(I32) == GUARD).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, msg=''):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)


def _coord_slack(rois, scale):
    """delta of tests/test_pointrend_gpu.py: 4 eps32 M scale, M the largest corner or extent."""
    r = np.abs(rois[:, 1:].astype(F64))
    M = max(float(r.max()), float(np.abs(rois[:, 3] - rois[:, 1]).max()), float(np.abs(rois[:, 4] - rois[:, 2]).max()), 1.0)
    return 4 * EPS32 * M * scale


# ---- point_features_bwd ---------------------------------------------------------------------------------------------------------------------
def _run_bwd(c, prior):
    from chainer_maskrcnn._hip import ops
    rows, P = c['coords'].shape[:2]
    outs = []
    for _ in range(2):
        buf, view = _guarded(prior)
        out = ops.point_features_bwd(_t(c['g_in']).view(rows, 1, P, -1), _t(c['coords']), _t(c['rois']), SCALE, view)
        torch.cuda.synchronize()
        assert out.data_ptr() == view.data_ptr() and _guard_ok(buf, prior.size)
        outs.append(view.cpu().numpy())
    _same_bits(outs[0], outs[1], 'two runs')
    return outs[0]


@pytest.mark.parametrize('name', cases.BWD_CASES)
def test_features_backward(name):
    c = cases.feature_cases()[name]
    args = (c['coords'], c['rois'], SCALE)
    delta = _coord_slack(c['rois'], SCALE)
    zero = np.zeros_like(c['g_map'])
    n_taps = pr.features_bwd(np.ones_like(c['g_in']), *args, zero, F64, unit_weights=True)
    g_taps = sum(pr.features_bwd(np.abs(c['g_in']), *args, zero, dt, unit_weights=True).astype(F64) for dt in (F32, F64))
    for prior in (zero, c['g_map']):
        got = _run_bwd(c, prior)
        _same_bits(got, pr.features_bwd(c['g_in'], *args, prior, F32), name)
        finite = np.isfinite(prior)
        safe = np.where(finite, prior, 0)
        b64 = pr.features_bwd(c['g_in'], *args, safe, F64)
        babs = pr.features_bwd(np.abs(c['g_in']), *args, np.abs(safe), F64)
        bound = (n_taps + 3) * EPS32 * babs + 2 * delta * g_taps
        err = np.abs(np.where(finite, got, 0).astype(F64) - b64)
        print('bwd %s, prior %s: worst err / bound %.3f, %d cells touched, at most %d taps on one' % (
            name, bool(prior.any()), float((err / np.maximum(bound, 1e-300)).max()), int((n_taps[..., 0] > 0).sum()), int(n_taps.max())))
        assert (err <= bound).all()
        _same_bits(got[n_taps == 0], prior[n_taps == 0], 'cells no tap lands on keep their bits')
        assert (got != prior).any() == bool(n_taps.any())


def test_features_backward_refuses_516_channels():
    from chainer_maskrcnn import _hip
    c = cases.feature_cases()[cases.BWD_REFUSED]
    from chainer_maskrcnn._hip import ops
    buf, view = _guarded(c['g_map'])
    with pytest.raises(_hip.MrcnnHipError, match='516 channels'):
        ops.point_features_bwd(_t(c['g_in']).view(5, 1, 7, -1), _t(c['coords']), _t(c['rois']), SCALE, view)
    torch.cuda.synchronize()
    _same_bits(view.cpu().numpy(), c['g_map'])
    assert _guard_ok(buf, c['g_map'].size)


# ---- point_features_fwd ---------------------------------------------------------------------------------------------------------------------
def _run_fwd(c):
    from chainer_maskrcnn._hip import ops
    args = (_t(c['coords']), _t(c['rois']), _t(c['fmap']), SCALE, _t(c['coarse']), c['n_fg'], c['cin_p'])
    got_t = ops.point_features_fwd(*args)
    torch.cuda.synchronize()
    assert torch.equal(ops.point_features_fwd(*args).view(I32), got_t.view(I32))
    rows, P = c['coords'].shape[:2]
    assert got_t.shape == (rows, 1, P, c['cin_p'])
    return got_t.cpu().numpy().reshape(rows, P, -1)


@pytest.mark.parametrize('name', cases.FWD_CASES)
def test_features_forward(name):
    c = cases.feature_cases()[name]
    C, n_fg = c['fmap'].shape[3], c['n_fg']
    fmap = c['fmap']
    a = (c['coords'], c['rois'], fmap, SCALE, c['coarse'], n_fg, c['cin_p'])
    got = _run_fwd(c)
    _same_bits(got, pr.features_fwd(*a, F32), name)
    w64 = pr.features_fwd(*a, F64)
    sabs = pr.features_fwd(c['coords'], c['rois'], np.abs(fmap), SCALE, np.abs(c['coarse']), n_fg, c['cin_p'], F64)
    bound = 4 * EPS32 * sabs
    bound[..., :C] += 4 * _coord_slack(c['rois'], SCALE) * float(np.abs(fmap).max())
    bound[..., C:] += 4 * (2 * EPS32 * c['coarse'].shape[1]) * float(np.abs(c['coarse']).max())
    err = np.abs(got.astype(F64) - w64)
    print('fwd %s: worst err / bound %.3f' % (name, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert not got[..., C + n_fg:].any() and got[..., C:C + n_fg].any()         # zeros behind the logical channels, whatever the padding holds
    bad = (c['rois'][:, 0] < 0) | (c['rois'][:, 0] >= c['fmap'].shape[0])
    assert not got[bad][..., :C].any() and (not bad.any() or got[bad][..., C:C + n_fg].all())


def test_features_forward_second_grid_pass():
    c = cases.second_pass_case()
    got = _run_fwd(c)
    want = pr.features_fwd(c['coords'], c['rois'], c['fmap'], SCALE, c['coarse'], c['n_fg'], c['cin_p'], F32)
    _same_bits(got[0], want[0])
    _same_bits(got[-1], want[-1])
    _same_bits(got, want)
    assert got[-1, :, 4].all() and got[-1, :, :4].any()


# ---- point_concat_fwd / point_concat_bwd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c0,n_coarse', cases.CONCAT_COARSE)
@pytest.mark.parametrize('Ch', cases.CONCAT_CH)
def test_concat_equals_slicing(Ch, c0, n_coarse):
    from chainer_maskrcnn._hip import ops
    for ld0, cin_p in cases.concat_shapes(Ch, c0, n_coarse):
        for n in cases.CONCAT_POINTS:
            c = cases.concat_case(Ch, c0, n_coarse, ld0, cin_p, n)
            h, x0, g_in = _t(c['h']).view(n, 1, 1, Ch), _t(c['x0']).view(n, 1, 1, ld0), _t(c['g_in']).view(n, 1, 1, cin_p)
            got = ops.point_concat_fwd(h, x0, c0, n_coarse, cin_p)
            g_h = ops.point_concat_bwd(g_in, Ch)
            torch.cuda.synchronize()
            assert got.shape == (n, 1, 1, cin_p) and g_h.shape == (n, 1, 1, Ch)
            _same_bits(got.cpu().numpy().reshape(n, cin_p), pr.concat_fwd(c['h'], c['x0'], c0, n_coarse, cin_p), str((ld0, cin_p, n)))
            _same_bits(g_h.cpu().numpy().reshape(n, Ch), pr.concat_bwd(c['g_in'], Ch), str((ld0, cin_p, n)))
            assert torch.equal(ops.point_concat_fwd(h, x0, c0, n_coarse, cin_p).view(I32), got.view(I32))
            assert torch.equal(ops.point_concat_bwd(g_in, Ch).view(I32), g_h.view(I32))
            # the guard behind out / g_h: through the library on buffers of this test's own
            lib, sp, p = _hip_handles()
            fill = np.zeros((n, cin_p), F32)
            buf, view = _guarded(fill)
            _hip_check(lib.mrcnn_point_concat_fwd(p(h), Ch, p(x0), ld0, c0, n_coarse, n, cin_p, p(view), sp()))
            buf2, view2 = _guarded(np.zeros((n, Ch), F32))
            _hip_check(lib.mrcnn_point_concat_bwd(p(g_in), cin_p, Ch, n, p(view2), sp()))
            torch.cuda.synchronize()
            assert torch.equal(view.view(I32), got.view(n, cin_p).view(I32)) and _guard_ok(buf, fill.size)
            assert torch.equal(view2.view(I32), g_h.view(n, Ch).view(I32)) and _guard_ok(buf2, n * Ch)


def _hip_handles():
    from chainer_maskrcnn import _hip
    return _hip.lib(), _hip.stream_ptr, _hip.ptr


def _hip_check(rc):
    from chainer_maskrcnn import _hip
    _hip.check(rc)


# ---- point_train_coords ---------------------------------------------------------------------------------------------------------------------
def _run_coords(c):
    from chainer_maskrcnn._hip import ops
    a = (_t(c['keys']), _t(c['coarse']), _t(c['label']), c['n_fg'], c['P'], c['n_cand'], c['n_imp'])
    got = ops.point_train_coords(*a)
    torch.cuda.synchronize()
    assert torch.equal(ops.point_train_coords(*a).view(I32), got.view(I32))
    return got.cpu().numpy()


@pytest.mark.parametrize('n_cand', cases.COORD_CANDS)
def test_train_coords_at_every_sort_size(n_cand):
    for P in cases.COORD_P:
        for S0 in cases.COORD_S0:
            for full in (False, True):
                c = cases.coords_case(n_cand, P, S0, full)
                got = _run_coords(c)
                want, picked = pr.train_coords(c['keys'], c['coarse'], c['label'], c['n_fg'], P, n_cand, c['n_imp'])
                _same_bits(got, want, str((n_cand, P, S0, full)))
                assert got.shape == (3, P, 2) and float(got.min()) >= 0 and float(got.max()) < 1
                np.testing.assert_array_equal(picked[2], np.arange(c['n_imp']))             # no channel: index order


def test_train_coords_refuses_4097_candidates():
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    keys = torch.zeros((1, 2 * 4097 + 2), dtype=I32, device=DEV)
    with pytest.raises(_hip.MrcnnHipError, match='4097 candidates'):
        ops.point_train_coords(keys, torch.zeros((1, 4, 4, 32), device=DEV), torch.ones((1,), dtype=I32, device=DEV), 3, 1, 4097, 0)
    torch.cuda.synchronize()


def test_train_coords_rank_zeros_first_and_nan_last():
    c = cases.special_coords_case()
    got = _run_coords(c)
    want, picked = pr.train_coords(c['keys'], c['coarse'], c['label'], c['n_fg'], c['P'], c['n_cand'], c['n_imp'])
    _same_bits(got, want)
    assert (got[1] == F32(1.0 - 2.0 ** -24)).all()


# ---- point_subdivide / point_scatter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', cases.SUB_S)
def test_subdivide_and_scatter(S):
    from chainer_maskrcnn._hip import ops
    c = cases.subdivide_case(S)
    D, cells = 5, 4 * S * S
    chosen = cases.chosen_grids(c)
    zero_label = dict(c, label=cases.chosen_channel(c['label'], c['n_channels']).astype(np.int32))
    for n_points in (1, cells, cells + 5):
        n_sel = min(n_points, cells)
        a = (_t(c['grid']), _t(c['label']), c['n_channels'], n_points)
        up, index, coords = ops.point_subdivide(*a)
        torch.cuda.synchronize()
        w_up, w_index, w_coords = pr.subdivide(chosen, n_points)
        assert up.shape == (D, 2 * S, 2 * S) and index.shape == (D, n_sel) and coords.shape == (D, n_sel, 2)
        np.testing.assert_array_equal(up.cpu().numpy(), w_up)               # NaN equals NaN here: its sign is the host's or the device's
        np.testing.assert_array_equal(index.cpu().numpy(), w_index)
        _same_bits(coords.cpu().numpy(), w_coords)
        np.testing.assert_array_equal(w_index[1], np.arange(n_sel))
        again = ops.point_subdivide(*a)
        assert all(torch.equal(x.view(I32), y.view(I32)) for x, y in zip(again, (up, index, coords)))
        # labels -1 and n_channels give what label 0 gives
        z = ops.point_subdivide(_t(c['grid']), _t(zero_label['label']), c['n_channels'], n_points)
        assert all(torch.equal(x.view(I32), y.view(I32)) for x, y in zip(z, (up, index, coords)))
        fin = np.isfinite(chosen)
        up64 = np.stack([pr.upsample2x(np.where(f, g, 0), F64) for g, f in zip(chosen, fin)])
        abs64 = np.stack([pr.upsample2x(np.where(f, np.abs(g), 0), F64) for g, f in zip(chosen, fin)])
        ok = np.isfinite(w_up)
        assert (np.abs(np.where(ok, up.cpu().numpy(), 0).astype(F64) - up64)[ok] <= (4 * EPS32 * abs64)[ok]).all()
        # scatter: the cells of the selection take the prediction of the label's channel (0 for a label without one)
        rs = np.random.RandomState(S + n_points)
        pred = rs.standard_normal((D, 1, n_sel, c['grid'].shape[3])).astype(F32)
        start = np.where(np.isfinite(w_up), w_up, 0).astype(F32)
        ch = cases.chosen_channel(c['label'], c['n_channels'])
        for idx in (w_index, _with_bad_indices(w_index, cells)):
            buf, view = _guarded(start)
            ops.point_scatter(_t(pred), _t(c['label']), _t(idx), c['n_channels'], view)
            torch.cuda.synchronize()
            want = start.reshape(D, -1).copy()
            for d in range(D):
                good = (idx[d] >= 0) & (idx[d] < cells)
                want[d, idx[d][good]] = pred[d, 0, good, ch[d]]
            _same_bits(view.cpu().numpy().reshape(D, -1), want)
            assert _guard_ok(buf, start.size)


def _with_bad_indices(index, cells):
    """the selection with entries replaced by -1 and by ``cells``: those are skipped (each detection keeps its other entries)."""
    idx = index.copy()
    idx[:, 0] = -1
    idx[1::2, -1] = cells
    idx[0, idx.shape[1] // 2] = cells
    return idx


def test_subdivide_refuses_a_57_grid():
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    with pytest.raises(_hip.MrcnnHipError, match='57 x 57'):
        ops.point_subdivide(torch.zeros((1, 57, 57, 8), device=DEV), None, 1, 10)
    torch.cuda.synchronize()


# ---- point_target ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(1, 1), (1, 7)])
def test_target_on_one_line_masks(H, W):
    from chainer_maskrcnn._hip import ops
    c = cases.target_case(H, W)
    a = (c['masks'], c['n_gt'], c['rois'], c['gt_assign'], c['label'], c['n_pos'], c['n_sample'], c['rows'], c['coords'])
    outs = []
    for _ in range(2):
        o = ops.point_target(_t(c['masks']), _t(c['n_gt']), _t(c['rois']), _t(c['gt_assign']), _t(c['label']), _t(c['n_pos']), c['n_sample'],
                             c['rows'], _t(c['coords']))
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
    _same_bits(outs[0], outs[1])
    got = outs[0]
    _same_bits(got, pr.target(*a, F32))
    assert (np.abs(got.astype(F64) - pr.target(*a, F64)) <= 4 * EPS32 + 4 * _coord_slack(c['rois'], 1.0)).all()
    assert not got[1].any() and (got[5] == -1).all() and (got[0] > 0).any()


# ---- point_bce ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.BCE_CASES))
def test_bce(name):
    from chainer_maskrcnn._hip import ops
    rows, P, ld, n_fg = cases.BCE_CASES[name]
    c = cases.bce_case(rows, P, ld, n_fg)
    weight = 1.5
    a = (_t(c['pred']), _t(c['target']), _t(c['label']), n_fg)
    out_t, gx_t = ops.point_bce(*a, weight=weight)
    torch.cuda.synchronize()
    out, gx = out_t.cpu().numpy(), gx_t.cpu().numpy().reshape(rows, P, ld)
    w_loss, w_count, w_gx = pr.bce(c['pred'], c['target'], c['label'], n_fg, weight, dt=F64)
    _, _, f_gx = pr.bce(c['pred'], c['target'], c['label'], n_fg, weight, dt=F32)
    extra = (w_gx != 0) * (weight / w_count)
    rg = rtol_from(f_gx, w_gx, extra)
    print('bce %s: loss %.3e rel, gradient %.1f eps32 (bar %.1f)' % (name, abs(float(out[0]) - w_loss) / w_loss, ratio(gx, w_gx, extra) / EPS32,
                                                                    rg / EPS32))
    assert out[1] == w_count
    loss_close(out[0], w_loss)
    assert ratio(gx, w_gx, extra) <= rg
    assert not gx[w_gx == 0].any() and gx[w_gx != 0].all() and not gx[[1, 2, 3]].any()
    out2, gx2 = ops.point_bce(*a, weight=weight)
    assert torch.equal(out2.view(I32), out_t.view(I32)) and torch.equal(gx2.view(I32), gx_t.view(I32))
