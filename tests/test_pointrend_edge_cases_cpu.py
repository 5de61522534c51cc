"""Every case of tests/pointrend_edge_cases.py is what it is named for - which 64-row block first touches a patch, how many taps a cell
receives, how many lane trips and grid passes a size takes, where the special values rank - asserted from the module's plain arithmetic
and from tests/pointrend_reference.py alone, on any machine.  A case that misses its path fails HERE instead of silently weakening
tests/test_pointrend_edges_gpu.py."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pointrend_reference as pr  # noqa: E402
from tests import pointrend_edge_cases as cases  # noqa: E402
from tests.pointrend_edge_cases import F32, F64, SCALE  # noqa: E402

CSRC = os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc')


def test_the_module_restates_the_constants_of_the_kernel_files():
    src = open(os.path.join(CSRC, 'pointrend.hip')).read()
    loss = open(os.path.join(CSRC, 'loss_common.h')).read()
    common = open(os.path.join(CSRC, 'common.h')).read()
    assert int(re.search(r'constexpr int NT = (\d+);', loss).group(1)) == cases.NT
    assert int(re.search(r'constexpr int MAXB = (\d+);', loss).group(1)) == cases.LOSS_BLOCKS
    assert int(re.search(r'constexpr int kWave = (\d+);', common).group(1)) == cases.WAVE
    assert 'constexpr int PB_H = %d, PB_W = %d, PB_CELLS = PB_H * PB_W, PB_WAVES = NT / 64;' % (cases.PB_H, cases.PB_W) in src
    assert int(re.search(r'constexpr int PT_MAX_CAND = (\d+);', src).group(1)) == cases.PT_MAX_CAND
    assert int(re.search(r'constexpr int SD_T = (\d+);', src).group(1)) == cases.SD_T
    assert 'constexpr int SD_MAX_CELLS = 112 * 112;' in src and (2 * cases.SD_MAX_S) ** 2 == 112 * 112
    assert 'if (lds > 64 * 1024)' in src and cases.LDS_BYTES == 64 * 1024
    assert 'std::min<long long>((n + NT - 1) / NT, %d)' % cases.GRID_CAP in src
    for loop in ('for (int r0 = 0; r0 < rows; r0 += 64)', 'for (int p0 = 0; p0 < P; p0 += 64)', 'for (int q = lane; q < C4; q += 64)',
                 'for (int q = lane; q < cin4; q += 64)', 'if (patch >= n_patches) return;', 'pt += (long long)gridDim.x * (NT / 64)'):
        assert loop in src, loop


def test_sizes_leave_the_first_trip_of_every_loop():
    # what tests/test_pointrend_gpu.py reaches: five rows, C <= 256, patches a multiple of four, one grid pass
    assert cases.ballot_trips(5) == 1 and cases.lane_trips(256) == 1 and cases.bwd_idle_waves(2, 9, 13) == 0 and cases.bwd_idle_waves(2, 16, 24) == 0
    assert cases.fwd_passes(5 * 196) == 1 and cases.loss_trips(1500 * 7) == 1           # (its gradient phase strides there: 96 columns a point)
    # what this pin reaches
    assert [cases.ballot_trips(r) for r in (65, 130)] == [2, 3] and cases.ballot_trips(65) == 2         # rows; the points of 'ordered sum'
    assert [cases.lane_trips(C) for C in (4, 260, 512, 516)] == [1, 2, 2, 3]
    assert cases.bwd_lds_bytes(512) == cases.LDS_BYTES and cases.bwd_lds_bytes(516) > cases.LDS_BYTES
    assert cases.n_patches(1, 1, 1) == 1 and cases.n_patches(1, 2, 4) == 1 and cases.n_patches(1, 5, 5) == 6
    assert [cases.bwd_idle_waves(1, h, w) for h, w in ((1, 1), (2, 4), (5, 5))] == [3, 3, 2]
    assert 5 % cases.PB_H and 5 % cases.PB_W                    # edge patches of the 5 x 5 map are cropped in both directions
    c = cases.second_pass_case()
    n = c['coords'].shape[0] * c['coords'].shape[1]
    assert n == 1400 * 196 > 4 * 65535 and cases.fwd_grid(n) == cases.GRID_CAP and cases.fwd_passes(n) == 2
    rows, P, ld, n_fg = cases.BCE_CASES['strided']
    assert rows * P > 1024 * 256 and cases.loss_trips(rows * P) == 2 and cases.loss_trips(rows * P * ld) == 5
    assert [cases.sort_size(n) for n in cases.COORD_CANDS] == [2, 2, 256, 512, 4096]                    # padding keys: 1, 0, 0, 255, 0
    assert cases.sort_size(cases.PT_MAX_CAND) == cases.PT_MAX_CAND
    assert 4 * cases.SD_MAX_S ** 2 == 112 * 112 and 4 * 57 ** 2 > 112 * 112


def _first_rows(t):
    """patch -> the first row that lands a tap on it."""
    first = {}
    for p, r in zip(t['patch'], t['row']):
        first.setdefault(int(p), int(r))
    return first


@pytest.mark.parametrize('rows', [65, 130])
def test_row_ballot_cases_cross_the_64_row_blocks(rows):
    c = cases.feature_cases()['ballot rows %d' % rows]
    assert c['rois'].shape == (rows, 5) and c['coords'].shape == (rows, 7, 2) and c['fmap'].shape == (2, 9, 13, 32)
    t = cases.tap_table(c)
    blocks = {}
    for p, r in zip(t['patch'], t['row']):
        blocks.setdefault(int(p), set()).add(int(r) // 64)
    assert any(len(b) > 1 for b in blocks.values())             # a patch with taps from rows of two 64-row blocks
    assert any(r >= 64 for r in _first_rows(t).values())        # a patch a row of a later block touches first
    if rows == 130:
        assert any(2 in b and len(b) > 1 for b in blocks.values())


def test_ordered_sum_case_piles_taps_on_a_cell():
    c = cases.feature_cases()['ordered sum']
    assert c['coords'].shape == (130, 65, 2) and (c['rois'] == c['rois'][0]).all()
    n = cases.taps_per_cell(c)
    assert n.max() > 500 and not n[1].any()
    # the order matters: the float32 sum in another order gives other bits
    fwd = pr.features_bwd(c['g_in'], c['coords'], c['rois'], SCALE, c['g_map'], F32)
    rev = pr.features_bwd(c['g_in'][::-1], c['coords'][::-1], c['rois'][::-1], SCALE, c['g_map'], F32)
    assert (fwd != rev).any()


def test_channel_and_geometry_cases():
    fc = cases.feature_cases()
    assert [fc[k]['g_in'].shape[2] - fc[k]['fmap'].shape[3] for k in ('channels 4 ld 32', 'channels 260 ld 260', 'channels 512 ld 544')] == [28, 0, 32]
    for k in ('map 1x1', 'map 2x4', 'map 5x5'):
        t = cases.tap_table(fc[k])
        N, H, W = fc[k]['fmap'].shape[:3]
        assert N == 1 and set(t['patch']) == set(range(cases.n_patches(1, H, W))), k           # every patch is touched
    c = fc['image 1 untouched']
    t = cases.tap_table(c)
    assert c['fmap'].shape[0] == 3 and set(t['img']) == {0, 2}                                  # no tap on image 1
    assert (c['g_map'][1].view(np.uint32) == cases.NAN_PAYLOAD).all() and np.isnan(c['g_map'][1]).all()
    assert np.isfinite(c['g_map'][[0, 2]]).all()


def test_box_cases():
    fc = cases.feature_cases()
    c = fc['boxes']
    r = c['rois']
    assert r[0, 3] < r[0, 1] and r[0, 4] < r[0, 2] and (r[1, 1:3] == r[1, 3:5]).all()
    X, Y = pr.frame(r, c['coords'], F32)
    _, _, w = pr.taps(X * F32(SCALE), Y * F32(SCALE), 13, 9, F32)
    assert (w[0][2] == 1).all() and not any(w[k][2].any() for k in (1, 2, 3))                   # lx == ly == 0 on the centre row
    t = cases.tap_table(c)
    assert set(t['row']) == {0, 1, 2, 3, 4}                                                     # every such box still lands taps
    c = fc['outside']
    assert c['rois'][:, 0].tolist() == [0, 1, 0, 1, -1, 2] and c['fmap'].shape[0] == 2
    assert len(cases.tap_table(c)['row']) == 0 and len(cases.tap_table(c, F64)['row']) == 0     # no tap inside
    np.testing.assert_array_equal(pr.features_bwd(c['g_in'], c['coords'], c['rois'], SCALE, c['g_map'], F32), c['g_map'])
    # the four boxes that miss the map do so geometrically, not by their image index
    inside = dict(c, rois=c['rois'].copy())
    inside['rois'][4:, 0] = (0, 1)
    assert set(cases.tap_table(inside)['row']) == {4, 5}
    c = fc['huge box']
    assert np.abs(c['rois'][:2, 1:]).min() == 1e9
    X, Y = pr.frame(c['rois'], c['coords'], F32)
    x0, y0, _ = pr.taps(X * F32(SCALE), Y * F32(SCALE), 13, 9, F32)
    assert x0[:2].min() == -2 and x0[:2].max() == 13 and y0[:2].min() == -2 and y0[:2].max() == 9      # both clamps
    for k in cases.BWD_CASES + cases.FWD_CASES + (cases.BWD_REFUSED,):
        assert (fc[k]['rois'][:, 0] == np.round(fc[k]['rois'][:, 0])).all(), k                  # no fractional image index


def test_forward_cases():
    fc = cases.feature_cases()
    c = fc['outside']
    w = pr.features_fwd(c['coords'], c['rois'], c['fmap'], SCALE, c['coarse'], c['n_fg'], c['cin_p'], F32)
    C = c['fmap'].shape[3]
    assert not w[4:, :, :C].any() and w[4:, :, C:C + c['n_fg']].all()           # index outside [0, N): no fine part, the coarse part sampled
    seen = set()
    for k in cases.FWD_CASES:
        if not k.startswith('coarse'):
            continue
        c = fc[k]
        C, n_fg, cin_p, S0 = c['fmap'].shape[3], c['n_fg'], c['cin_p'], c['coarse'].shape[1]
        assert c['coarse'].all() and c['coarse'].shape[3] > n_fg                # data in every padded channel
        assert cin_p == cases.ceil4(C + n_fg) + (0 if n_fg == 4 else 8)
        seen.add((n_fg, S0, (C + n_fg) % 4, cin_p == C + n_fg))
    assert seen == {(1, 1, 1, False), (2, 7, 2, False), (4, 1, 0, True), (5, 7, 1, False), (80, 1, 0, False)}
    assert fc['channels 516']['cin_p'] >= 516 + 3


def test_concat_shapes_are_the_smallest_legal_and_larger():
    for Ch in cases.CONCAT_CH:
        for c0, nco in cases.CONCAT_COARSE:
            shapes = cases.concat_shapes(Ch, c0, nco)
            ld0, cin_p = shapes[0]
            assert ld0 % 4 == 0 and cin_p % 4 == 0 and c0 % 4 == 0
            assert ld0 - 4 < c0 + nco <= ld0 and cin_p - 4 < Ch + nco <= cin_p              # one float4 less is refused by the entry point
            assert {s[0] > ld0 for s in shapes} == {False, True} and {s[1] > cin_p for s in shapes} == {False, True}
    c = cases.concat_case(4, 256, 3, 260, 8, 1000)
    w = pr.concat_fwd(c['h'], c['x0'], 256, 3, 8)
    assert w[:, :4].tolist() == c['h'].tolist() and w[:, 4:7].tolist() == c['x0'][:, 256:259].tolist() and not w[:, 7].any() and c['x0'][:, 259].all()
    assert pr.concat_bwd(c['g_in'], 4).tolist() == c['g_in'][:, :4].tolist()


def test_train_coords_cases():
    combos = [(n, P, S0, full) for n in cases.COORD_CANDS for P in cases.COORD_P for S0 in cases.COORD_S0 for full in (False, True)]
    assert len(combos) == 40
    for n, P, S0, full in combos:
        c = cases.coords_case(n, P, S0, full)
        assert c['n_imp'] == (min(P, n) if full else 0) and c['keys'].shape[1] == 2 * n + 2 * (P - c['n_imp']) and c['coarse'].shape[1] == S0
    c = cases.special_coords_case()
    row = c['coarse'][0, :, :, c['label'][0] - 1]
    bits = set(row.view(np.uint32).reshape(-1).tolist())
    assert {0x80000000, 0x7f800000, 0xff800000, 0x7fc00000} <= bits and (np.abs(row[np.isfinite(row) & (row != 0)]) < np.finfo(F32).tiny).all()
    val = pr.candidate_values(c['keys'], c['coarse'], c['label'], c['n_fg'], c['n_cand'])
    order = pr.rank(val[0])
    zeros = np.nonzero(val[0] == 0)[0]
    assert len(zeros) > 10 and order[:len(zeros)].tolist() == zeros.tolist()                # the zero and -0.0 candidates first, in index order
    x = pr.key_unit(c['keys'])[0, 0:512:2] * F32(8)
    assert (x[zeros] < 2.5).all() and (x[zeros] > 1.5).any() and (x[zeros] < 1.0).any()     # candidates on the -0.0 columns among them
    assert np.isnan(val[0][order[-1]]) and np.isinf(val[0]).any()                           # a NaN candidate last, behind the infinities
    n_nan = int(np.isnan(val[0]).sum())
    assert np.isnan(val[0][order[-n_nan:]]).all() and order[-n_nan:].tolist() == sorted(order[-n_nan:].tolist())
    denorm = (val[0] != 0) & (np.abs(val[0]) < np.finfo(F32).tiny)
    assert denorm.any() and (np.abs(val[0][denorm]).view(np.uint32) < 0x00800000).all()
    want, picked = pr.train_coords(c['keys'], c['coarse'], c['label'], c['n_fg'], c['P'], c['n_cand'], c['n_imp'])
    assert (want[1] == F32(1.0 - 2.0 ** -24)).all()                                        # keys with all bits set
    assert sorted(picked[0].tolist()) == list(range(256)) and picked[0].tolist() == order.tolist()
    # for finite input the bit ranking is the ranking by |value|
    v = val[2]
    assert np.isfinite(v).all() and pr.rank(v).tolist() == np.argsort(np.abs(v), kind='stable').tolist()


@pytest.mark.parametrize('S', cases.SUB_S)
def test_subdivide_cases(S):
    c = cases.subdivide_case(S)
    g = cases.chosen_grids(c)
    assert not g[1].any()
    assert (c['grid'][[0, 2, 3, 4]] != 0).all()                                            # also the channels the last two labels must not select
    np.testing.assert_array_equal(g[3], c['grid'][3, :, :, 0])
    np.testing.assert_array_equal(g[4], c['grid'][4, :, :, 0])
    assert not np.isfinite(g[2]).all()
    if S > 1:
        assert np.isnan(g[2]).any() and np.isposinf(g[2]).any() and np.isneginf(g[2]).any()
    for n_sel in (1, 4 * S * S):
        up, index, coords = pr.subdivide(g, n_sel)
        assert index.shape == (5, n_sel) and index[1].tolist() == list(range(n_sel))       # all equal: the tie rule alone fills the slots
        assert (np.diff(index, axis=1) > 0).all()
        if n_sel < 4 * S * S and S > 1:
            assert np.isfinite(up[2].reshape(-1)[index[2]]).all()                          # inf and NaN rank behind every finite cell
    assert pr.subdivide(g, 4 * S * S + 5)[1].shape == (5, 4 * S * S)                       # the clamp of ops.point_subdivide
    assert S % 2 == 1 or S == 56


@pytest.mark.parametrize('H,W', [(1, 1), (1, 7)])
def test_target_cases(H, W):
    c = cases.target_case(H, W)
    assert c['masks'].shape == (3, 1, H, W) and c['rows'] < c['n_sample'] and c['coords'].shape[1] == 196 and W % 2 == 1
    a = (c['masks'], c['n_gt'], c['rois'], c['gt_assign'], c['label'], c['n_pos'], c['n_sample'], c['rows'], c['coords'])
    live = pr.live_rows(c['n_gt'], c['gt_assign'], c['label'], c['n_pos'], c['n_sample'], c['rows'], 1)
    w = pr.target(*a, F32)
    assert live.tolist() == [True, True, True, True, True, False]
    assert live[1] and not w[1].any() and c['masks'][0].all()                              # a live row whose target is all zero
    assert (w[0] > 0).any() and (w[5] == -1).all()


@pytest.mark.parametrize('name', sorted(cases.BCE_CASES))
def test_bce_cases(name):
    rows, P, ld, n_fg = cases.BCE_CASES[name]
    c = cases.bce_case(rows, P, ld, n_fg)
    loss, count, gx = pr.bce(c['pred'], c['target'], c['label'], n_fg, 1.0, dt=F64)
    assert c['label'][3] == n_fg + 1 and (c['target'][3] >= 0).all() and not gx[3].any()   # skipped: no gradient, not counted
    counted = (c['target'] >= 0) & ((c['label'] >= 1) & (c['label'] <= n_fg))[:, None]
    assert count == counted.sum() and not counted[[1, 2, 3]].any() and count > 0
    if name == 'one point':
        assert P == 1 and ld > n_fg and c['pred'][3, 0, :, n_fg].all()                     # the column its label names is real data
