"""GPU tests: csrc/nn.hip at the edges of its plans, against float64 (tests/nn_cases.py).

The BatchNorm reductions run every case of the table - per-thread row counts on both sides of the in-flight loops, P of 1, 2, 3, a last
block with a single row, block counts on both sides of the finaliser's 64 / 256 slices, a binding cap - with both finaliser layouts
(mrcnn_debug_bn_plan fin_quads 4 and 1); the finaliser also takes hand-made partial rows, its exact recompute its own loop edges, and
the shifted statistics pass a first row far from the channel's mean.  The layer kernels run one shape just past the 1,048,576 float4
groups one trip of their grid-stride loop covers, and one small ragged shape."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import nn_cases as nc

pytestmark = pytest.mark.gpu

from chainer_maskrcnn import _hip  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn._hip.nn import workspace  # noqa: E402

DEV = 'cuda:0'
EPS32 = float(np.finfo(np.float32).eps)
QUADS = (4, 1)


@pytest.fixture(scope='module', autouse=True)
def _shipped_plan_afterwards():
    """tests/conftest.py does not reset mrcnn_debug_bn_plan: whatever happens in this module, the shipped plan is back afterwards."""
    try:
        yield
    finally:
        _hip.check(_hip.lib().mrcnn_debug_bn_plan(nc.SHIPPED_CAP, 4))


@contextlib.contextmanager
def _plan(red_cap, fin_quads):
    _hip.check(_hip.lib().mrcnn_debug_bn_plan(red_cap, fin_quads))
    try:
        yield
    finally:
        _hip.check(_hip.lib().mrcnn_debug_bn_plan(nc.SHIPPED_CAP, 4))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(_n(got).astype(np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-6)


class _Bars:
    """Collects (name, err, floor, bar); a line per check is printed, the failures are asserted at the end of the test."""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def check(self, name, got, ref, bar, ref32=None):
        err = _err(got, ref)
        floor = None
        if ref32 is not None:            # an ill-conditioned case: the same expression in float32, in the kernel's order
            floor = float(np.abs(np.asarray(ref32, np.float64) - np.asarray(ref, np.float64)).max()) / max(float(np.abs(ref).max()), 1e-6)
            bar = max(bar, 3 * floor)
        key = name.split('/')[-1]
        if err >= self.worst.get(key, (-1.0,))[0]:
            self.worst[key] = (err, floor, bar, name)
        if not err <= bar:
            self.bad.append((name, err, floor, bar))

    def done(self):
        for key, (err, floor, bar, name) in sorted(self.worst.items()):
            print('%-24s %-10s err %.3e floor %s bar %.1e (%s)' % (self.case, key, err, 'none     ' if floor is None else '%.3e' % floor, bar, name))
        assert not self.bad, self.bad


def test_the_restated_plan_is_the_librarys_plan():
    lib = _hip.lib()
    for case in nc.PLAN_CASES:
        for cap in {case.red_cap, nc.SHIPPED_CAP, 3}:
            with _plan(cap, 4):
                assert lib.mrcnn_bn_workspace_bytes(case.P, case.C) == nc.workspace_bytes(case.P, case.C, cap), (case, cap)
                assert lib.mrcnn_bn_pair_workspace_bytes(case.P, case.C) == nc.workspace_bytes(case.P, case.C, cap, stats=3), (case, cap)
    for P, C in [(2 * 256 * 256, 256), (129 * 128, 256), (2064, 2048), (509, 20), (8192, 64), (1, 4)]:
        assert lib.mrcnn_bn_workspace_bytes(P, C) == nc.workspace_bytes(P, C)
        assert lib.mrcnn_bn_pair_workspace_bytes(P, C) == nc.workspace_bytes(P, C, stats=3)
    assert lib.mrcnn_bn_workspace_bytes(4, 6) == 0 and lib.mrcnn_bn_workspace_bytes(0, 8) == 0


def _stats_only(x, P, C, part=None, run=None):
    """mrcnn_bn_train_stats_f32: (mean, invstd) without an apply kernel; run = (running_mean, running_var) updated in place."""
    lib, ptr = _hip.lib(), _hip.ptr
    m, s = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws = workspace(lib.mrcnn_bn_workspace_bytes(P, C), x.device)
    rm, rv = run if run is not None else (None, None)
    _hip.check(lib.mrcnn_bn_train_stats_f32(ptr(x), ptr(part), 0 if part is None else part.shape[0], ptr(m), ptr(s), ptr(rm), ptr(rv), P, C, nc.EPS,
                                            nc.DECAY, ptr(ws), ws.numel(), _hip.stream_ptr()))
    return m, s


def _pair_fwd(xa, ga, ba, xb, gb, bb, P, C):
    lib, ptr = _hip.lib(), _hip.ptr
    y = torch.empty_like(xa)
    ma, sa, mb, sb = (torch.empty(C, device=DEV) for _ in range(4))
    run = [torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]
    ws = workspace(lib.mrcnn_bn_workspace_bytes(P, C), xa.device)
    _hip.check(lib.mrcnn_bn_train_fwd_pair_f32(ptr(xa), None, 0, ptr(ga), ptr(ba), ptr(ma), ptr(sa), ptr(run[0]), ptr(run[1]), ptr(xb), None, 0, ptr(gb),
                                               ptr(bb), ptr(mb), ptr(sb), ptr(run[2]), ptr(run[3]), ptr(y), P, C, nc.EPS, nc.DECAY, ptr(ws), ws.numel(),
                                               _hip.stream_ptr()))
    return y, ma, sa, mb, sb, run


def _pair_bwd(gy, y, xa, xb, ga, ma, sa, gb, mb, sb, P, C):
    lib, ptr = _hip.lib(), _hip.ptr
    gxa, gxb = torch.empty_like(xa), torch.empty_like(xb)
    gga, gba, ggb, gbb = (torch.empty(C, device=DEV) for _ in range(4))
    ws = workspace(lib.mrcnn_bn_pair_workspace_bytes(P, C), xa.device)
    _hip.check(lib.mrcnn_bn_train_bwd_pair_f32(ptr(gy), ptr(y), ptr(xa), ptr(xb), ptr(ga), ptr(ma), ptr(sa), ptr(gb), ptr(mb), ptr(sb), ptr(gxa), ptr(gxb),
                                               ptr(gga), ptr(gba), ptr(ggb), ptr(gbb), P, C, ptr(ws), ws.numel(), _hip.stream_ptr()))
    return gxa, gxb, gga, gba, ggb, gbb


@pytest.mark.parametrize('case', nc.PLAN_CASES, ids=lambda c: c.name)
def test_bn_at_the_plan_edges(case):
    """Forward (plain, ReLU, residual + ReLU), the statistics-only call, backward (no ReLU; mask from y with and without the residual's
    gradient; mask recomputed from x) and the pair, with both finaliser layouts, against float64.  Bars of tests/test_nn_gpu.py: y 1e-5,
    mean 1e-6, invstd and running statistics 1e-5, gx / ggamma / gbeta 2e-5 of the tensor's maximum; for P <= 3 (gx is a difference of
    nearly equal terms) max(that, 3 x the error of the float32 restatement)."""
    P, C = case.P, case.C
    d = nc.plan_data(case)
    ill = P <= 3
    x64 = nc.f64(d['x'])
    mean, var, invstd = nc.bn_stats(d['x'])
    xhat = (x64 - mean) * invstd
    y_plain = nc.f64(d['gamma']) * xhat + nc.f64(d['beta'])
    want_y = {(False, False): y_plain, (True, False): np.maximum(y_plain, 0), (True, True): np.maximum(y_plain + nc.f64(d['res']), 0)}
    want_rm, want_rv = nc.running_stats(mean, var, P, np.zeros(C), np.ones(C))
    y_pair, sta, stb = nc.pair_forward(d['x'], d['gamma'], d['beta'], d['xb'], d['gamma_b'], d['beta_b'])
    f32 = {}
    if ill:
        for k, (relu, res) in enumerate(want_y):
            f32[(relu, res)] = nc.bn_forward_f32(d['x'], d['gamma'], d['beta'], d['res'] if res else None, relu)
    y_pair32 = None
    if ill:
        r32 = nc.bn_forward_f32(d['xb'], d['gamma_b'], d['beta_b'])[0]
        y_pair32 = nc.bn_forward_f32(d['x'], d['gamma'], d['beta'], r32, True)[0]
    t = {k: _t(v) for k, v in d.items()}
    bars = _Bars(case.name)
    bwd_refs = {}

    def bwd_ref(key, mask):
        """float64 backward with the mask the kernel saw (its own y) - shared between the finaliser layouts while that mask is the same"""
        hit = bwd_refs.get(key)
        if hit is None or not (mask is None or np.array_equal(hit[0], mask)):
            hit = (mask, nc.bn_backward(d['gy'], d['x'], d['gamma'], mean, invstd, mask))
            bwd_refs[key] = hit
        return hit[1]

    for fq in QUADS:
        with _plan(case.red_cap, fq):
            tag = 'q%d/' % fq
            ys = {}
            for relu, res in want_y:
                rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
                yd, m, s = ops.bn_train_fwd(t['x'], t['gamma'], t['beta'], t['res'] if res else None, relu, rm, rv)
                ys[(relu, res)] = (yd, m, s)
                r32 = f32.get((relu, res))
                bars.check(tag + 'fwd%d%d/y' % (relu, res), yd, want_y[(relu, res)], 1e-5, r32[0] if ill else None)
                bars.check(tag + 'fwd%d%d/mean' % (relu, res), m, mean, 1e-6, r32[1] if ill else None)
                bars.check(tag + 'fwd%d%d/invstd' % (relu, res), s, invstd, 1e-5, r32[2] if ill else None)
                bars.check(tag + 'fwd%d%d/run_mean' % (relu, res), rm, want_rm, 1e-5)
                bars.check(tag + 'fwd%d%d/run_var' % (relu, res), rv, want_rv, 1e-5)
            yd, m, s = ys[(True, False)]
            # the statistics-only call and a second forward: the same bits
            rm2, rv2 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
            m2, s2 = _stats_only(t['x'], P, C, run=(rm2, rv2))
            assert torch.equal(m2, m) and torch.equal(s2, s)
            bars.check(tag + 'stats/run_mean', rm2, want_rm, 1e-5)
            bars.check(tag + 'stats/run_var', rv2, want_rv, 1e-5)
            yd2, m3, s3 = ops.bn_train_fwd(t['x'], t['gamma'], t['beta'], None, True)
            assert torch.equal(yd2, yd) and torch.equal(m3, m) and torch.equal(s3, s)
            # backward: mode 0, mode 1 (mask read from y) with / without gres, mode 2 (mask recomputed from x)
            runs = [('bwd0', None, False, False, None), ('bwd1res', ys[(True, True)][0], True, True, None), ('bwd1', yd, True, False, None),
                    ('bwd2', None, True, False, t['beta'])]
            got1 = None
            for name, ymask, relu, gres_wanted, beta in runs:
                gx, gres, gg, gb = ops.bn_train_bwd(t['gy'], t['x'], ymask, t['gamma'], m, s, relu, gres_wanted, beta=beta)
                mask = None if not relu else _n(ymask if ymask is not None else yd) > 0
                rgx, rdz, rgg, rgb = bwd_ref(name, mask)
                r32 = nc.bn_backward_f32(d['gy'], d['x'], d['gamma'], _n(m), _n(s), mask) if ill else (None, None, None)
                bars.check(tag + name + '/gx', gx, rgx, 2e-5, r32[0])
                bars.check(tag + name + '/ggamma', gg, rgg, 2e-5, r32[1])
                bars.check(tag + name + '/gbeta', gb, rgb, 2e-5, r32[2])
                if gres_wanted:
                    np.testing.assert_array_equal(_n(gres), rdz.astype(np.float32))
                else:
                    assert gres is None
                if name == 'bwd1':
                    got1 = (gx, gg, gb)
                    again = ops.bn_train_bwd(t['gy'], t['x'], ymask, t['gamma'], m, s, relu, False)
                    assert torch.equal(again[0], gx) and torch.equal(again[2], gg) and torch.equal(again[3], gb)
                if name == 'bwd2':      # bitwise the gradients of the mask read from y
                    assert torch.equal(gx, got1[0]) and torch.equal(gg, got1[1]) and torch.equal(gb, got1[2])
            # the pair
            yp, ma, sa, mb, sb, run = _pair_fwd(t['x'], t['gamma'], t['beta'], t['xb'], t['gamma_b'], t['beta_b'], P, C)
            bars.check(tag + 'pair/y', yp, y_pair, 1e-5, y_pair32)
            bars.check(tag + 'pair/mean', ma, sta[0], 1e-6)
            bars.check(tag + 'pair/mean', mb, stb[0], 1e-6)
            bars.check(tag + 'pair/invstd', sa, sta[2], 1e-5)
            bars.check(tag + 'pair/invstd', sb, stb[2], 1e-5)
            rma, rva = nc.running_stats(sta[0], sta[1], P, np.zeros(C), np.ones(C))
            rmb, rvb = nc.running_stats(stb[0], stb[1], P, np.zeros(C), np.ones(C))
            for got, ref, nm in ((run[0], rma, 'run_mean'), (run[1], rva, 'run_var'), (run[2], rmb, 'run_mean'), (run[3], rvb, 'run_var')):
                bars.check(tag + 'pair/' + nm, got, ref, 1e-5)
            assert torch.equal(ma, m) and torch.equal(sa, s)
            yp2 = _pair_fwd(t['x'], t['gamma'], t['beta'], t['xb'], t['gamma_b'], t['beta_b'], P, C)[0]
            assert torch.equal(yp2, yp)
            maskp = _n(yp) > 0
            gy_masked = _t(np.where(maskp, d['gy'], np.float32(0)))
            key = 'pair'
            hit = bwd_refs.get(key)
            if hit is None or not np.array_equal(hit[0], maskp):
                hit = (maskp, nc.pair_backward(d['gy'], maskp, d['x'], d['gamma'], sta[0], sta[2], d['xb'], d['gamma_b'], stb[0], stb[2]))
                bwd_refs[key] = hit
            got_y = _pair_bwd(t['gy'], yp, t['x'], t['xb'], t['gamma'], ma, sa, t['gamma_b'], mb, sb, P, C)
            got_m = _pair_bwd(gy_masked, None, t['x'], t['xb'], t['gamma'], ma, sa, t['gamma_b'], mb, sb, P, C)
            r32 = [None] * 6
            if ill:
                a32 = nc.bn_backward_f32(d['gy'], d['x'], d['gamma'], _n(ma), _n(sa), maskp)
                b32 = nc.bn_backward_f32(d['gy'], d['xb'], d['gamma_b'], _n(mb), _n(sb), maskp)
                r32 = [a32[0], b32[0], a32[1], a32[2], b32[1], b32[2]]
            for nm, g1, g2, ref, flo in zip(('gx', 'gx', 'ggamma', 'gbeta', 'ggamma', 'gbeta'), got_y, got_m, hit[1], r32):
                bars.check(tag + 'pairbwd/' + nm, g1, ref, 2e-5, flo)
                assert torch.equal(g1, g2)
    bars.done()


def _stat_bars(name, mean, invstd, out, x, bad, lines):
    """The bars of test_bn_statistics_from_the_epilogue_with_a_large_mean, against the float64 two-pass statistics: invstd within 2e-5
    relative, mean within 2e-6 of its scale, the normalised output within 1e-4 of its scale.  No float32 floor here: a float32 restatement
    of the same sums shares their cancellation."""
    m64, v64, is64 = nc.bn_stats(x)
    e_is = np.abs(_n(invstd).astype(np.float64) - is64) / is64
    e_m = np.abs(_n(mean).astype(np.float64) - m64) / max(float(np.abs(m64).max()), 1e-30)
    want = (nc.f64(x) - m64) * is64
    e_o = float(np.abs(_n(out).astype(np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)
    lines.append('%-34s invstd %.3e (ch %d) mean %.3e out %.3e' % (name, e_is.max(), int(e_is.argmax()), e_m.max(), e_o))
    if not (e_is.max() <= 2e-5 and e_m.max() <= 2e-6 and e_o <= 1e-4):
        bad.append(lines[-1])
    return e_is


@pytest.mark.parametrize('rows,C', nc.PARTIAL_CASES)
def test_finaliser_on_hand_made_partials(rows, C):
    """reduce_partials on partial rows built on the host (rows of 1, 63..65, 255..257, 1024: both sides of 64 and 256 slices and of four
    rows in flight; C of 4, 8, 20: channel blocks partly outside), through bn_train_fwd_stats and the statistics-only call, both layouts."""
    P = nc.PARTIAL_P
    x = (np.random.RandomState(rows + C).standard_normal((P, C)) * 2 + 3).astype(np.float32)
    part = _t(nc.make_partials(x, rows))
    xt, one, zero = _t(x), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    m64, v64, _ = nc.bn_stats(x)
    want_rm, want_rv = nc.running_stats(m64, v64, P, np.zeros(C), np.ones(C))
    bad, lines = [], []
    for fq in QUADS:
        with _plan(nc.SHIPPED_CAP, fq):
            rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
            o, m, s = ops.bn_train_fwd_stats(xt, part, one, zero, None, False, rm, rv)
            _stat_bars('rows%d_C%d q%d' % (rows, C, fq), m, s, o, x, bad, lines)
            assert _err(rm, want_rm) <= 1e-5 and _err(rv, want_rv) <= 1e-5
            m2, s2 = _stats_only(xt, P, C, part=part)
            o2, m3, s3 = ops.bn_train_fwd_stats(xt, part, one, zero, None, False, None, None)
            assert torch.equal(m2, m) and torch.equal(s2, s) and torch.equal(m3, m) and torch.equal(s3, s) and torch.equal(o2, o)
    print('\n'.join(lines))
    assert not bad, bad


@pytest.mark.parametrize('P,ratio,C,only_one', nc.RECOMPUTE_CASES)
def test_exact_recompute_at_its_loop_edges(P, ratio, C, only_one):
    """k_bn_stats_final's exact pass (un-shifted partial rows take it past |mean| / std = 32: ratio 80 and 400; not at 20) with P on
    both sides of its eight rows in flight times 16 (fin_quads 4) or 64 (fin_quads 1) slices, a block where one channel of sixteen asks
    for it, C = 20 (lanes past C)."""
    x = nc.large_mean_data(P, ratio, C, only_one)
    part = _t(nc.make_partials(x, nc.recompute_rows(P)))
    xt, one, zero = _t(x), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    bad, lines = [], []
    for fq in QUADS:
        with _plan(nc.SHIPPED_CAP, fq):
            o, m, s = ops.bn_train_fwd_stats(xt, part, one, zero, None, False, None, None)
            _stat_bars('P%d_r%g_C%d%s q%d' % (P, ratio, C, '_one' if only_one else '', fq), m, s, o, x, bad, lines)
            o2, m2, s2 = ops.bn_train_fwd_stats(xt, part, one, zero, None, False, None, None)
            assert torch.equal(o2, o) and torch.equal(m2, m) and torch.equal(s2, s)
    print('\n'.join(lines))
    assert not bad, bad


def _first_row(P, C, sigmas):
    x, k = nc.first_row_data(P, C, sigmas)
    xt, one, zero = _t(x), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    bad, lines = [], []
    for fq in QUADS:
        with _plan(nc.SHIPPED_CAP, fq):
            o, m, s = ops.bn_train_fwd(xt, one, zero, None, False)
            e = _stat_bars('first_row P%d_C%d q%d' % (P, C, fq), m, s, o, x, bad, lines)
            for sg in sorted(set(np.abs(k[:C - 2]))):
                lines.append('    x[0] %6g sigma off: worst invstd error %.3e' % (sg, e[:C - 2][np.abs(k[:C - 2]) == sg].max()))
            lines.append('    std 1e-3 channel: %.3e, dead channel: %.3e' % (e[C - 2], e[C - 1]))
            m2, s2 = _stats_only(xt, P, C)
            assert torch.equal(m2, m) and torch.equal(s2, s)
    print('\n'.join(lines))
    assert not bad, bad


@pytest.mark.parametrize('P,C', nc.FIRST_ROW_SHAPES)
def test_shifted_statistics_with_a_first_row_far_from_the_mean(P, C):
    """The statistics pass shifts by K = x[0][c].  With x[0][c] 10 / 100 / 1000 standard deviations from the channel's mean (a nearly
    constant channel whose corner pixel differs), a dead channel and a channel of standard deviation 1e-3 whose first value is off by 1,
    the float32 sums of (x - K) and (x - K)^2 cancel as un-shifted ones do at a large mean: past |mean - K| / std = 8 the finaliser
    recomputes the channel exactly.  Before a guard covered the shifted sums this test measured 1 / sigma off by 1.5e-4 and the mean
    by 5.1e-6 of its scale at (8192, 64), 9.6e-5 and 3.7e-5 at (509, 20)."""
    _first_row(P, C, nc.FIRST_ROW_SIGMAS)


@pytest.mark.parametrize('P,C', nc.BELOW_GUARD_SHAPES)
def test_shifted_statistics_just_below_the_recompute_guard(P, C):
    """x[0][c] 5 and 7.5 standard deviations off: |mean - K| / std stays below the shifted sums' guard of 8, so the float32 sums
    themselves must hold the bars - also where one block adds the sums of 51 row lanes in float32 ((509, 20): the shape that set the
    guard; DESIGN.md section 3.5 has the errors measured at ratios 10, 22 and 30)."""
    x, k = nc.first_row_data(P, C, nc.BELOW_GUARD_SIGMAS)
    m64, v64, _ = nc.bn_stats(x)
    r = np.abs(m64 - x[0]) / np.sqrt(np.where(v64 > 0, v64, 1))
    assert 6.5 < r[:C - 2].max() < 8
    _first_row(P, C, nc.BELOW_GUARD_SIGMAS)


def test_dead_channel_through_forward_and_backward():
    """A channel whose values are all equal: variance 0, invstd = 1 / sqrt(eps), xhat = 0; bar max(the usual, 3 x the float32 floor)."""
    P, C = 509, 20
    rs = np.random.RandomState(3)
    x = (rs.standard_normal((P, C)) * 2 + 3).astype(np.float32)
    x[:, C - 1] = 1.25
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(np.float32), rs.standard_normal(C).astype(np.float32)
    gy = rs.standard_normal((P, C)).astype(np.float32)
    y64, mean, var, invstd = nc.bn_forward(x, gamma, beta, None, True)
    assert var[C - 1] == 0.0
    y32, m32, s32 = nc.bn_forward_f32(x, gamma, beta, None, True)
    bars = _Bars('dead_channel')
    for fq in QUADS:
        with _plan(nc.SHIPPED_CAP, fq):
            yd, m, s = ops.bn_train_fwd(_t(x), _t(gamma), _t(beta), None, True)
            bars.check('q%d/y' % fq, yd, y64, 1e-5, y32)
            bars.check('q%d/mean' % fq, m, mean, 1e-6, m32)
            bars.check('q%d/invstd' % fq, s, invstd, 1e-5, s32)
            assert _n(s)[C - 1] == np.float32(1) / np.sqrt(np.float32(nc.EPS)) and _n(m)[C - 1] == x[0, C - 1]
            mask = _n(yd) > 0
            gx, _, gg, gb = ops.bn_train_bwd(_t(gy), _t(x), yd, _t(gamma), m, s, True, False)
            rgx, _, rgg, rgb = nc.bn_backward(gy, x, gamma, mean, invstd, mask)
            r32 = nc.bn_backward_f32(gy, x, gamma, _n(m), _n(s), mask)
            bars.check('q%d/gx' % fq, gx, rgx, 2e-5, r32[0])
            bars.check('q%d/ggamma' % fq, gg, rgg, 2e-5, r32[1])
            bars.check('q%d/gbeta' % fq, gb, rgb, 2e-5, r32[2])
            assert _n(gg)[C - 1] == 0.0
    bars.done()


def test_channel_counts_the_reduction_passes_cannot_take_are_refused():
    """C / 4 above 256 and no multiple of 256: the channel loops of the three reduction passes hold barriers and would run a different
    number of trips per thread.  The five entry points that run such a pass return MRCNN_E_INVALID before any launch (the outputs keep
    their contents); the forms fed by partial rows take the count."""
    lib, ptr, sp = _hip.lib(), _hip.ptr, _hip.stream_ptr
    for C in (1028, 1536, 2044):
        assert nc.channels_refused(C)
        P = 2
        x = torch.ones((P, C), device=DEV)
        v = [torch.full((C,), 7.0, device=DEV) for _ in range(8)]
        out = torch.full((P, C), 7.0, device=DEV)
        out2 = torch.full((P, C), 7.0, device=DEV)
        ws = workspace(max(lib.mrcnn_bn_workspace_bytes(P, C), lib.mrcnn_bn_pair_workspace_bytes(P, C)), x.device)
        rcs = [lib.mrcnn_bn_train_fwd_f32(ptr(x), ptr(v[0]), ptr(v[1]), None, ptr(out), ptr(v[2]), ptr(v[3]), None, None, P, C, nc.EPS, nc.DECAY, 1, ptr(ws),
                                          ws.numel(), sp()),
               lib.mrcnn_bn_train_bwd_f32(ptr(x), ptr(x), ptr(x), ptr(v[0]), ptr(v[1]), ptr(v[0]), ptr(v[1]), ptr(out), None, ptr(v[2]), ptr(v[3]), P, C, 1,
                                          ptr(ws), ws.numel(), sp()),
               lib.mrcnn_bn_train_stats_f32(ptr(x), None, 0, ptr(v[2]), ptr(v[3]), None, None, P, C, nc.EPS, nc.DECAY, ptr(ws), ws.numel(), sp()),
               lib.mrcnn_bn_train_fwd_pair_f32(ptr(x), None, 0, ptr(v[0]), ptr(v[1]), ptr(v[2]), ptr(v[3]), None, None, ptr(x), None, 0, ptr(v[0]), ptr(v[1]),
                                               ptr(v[4]), ptr(v[5]), None, None, ptr(out), P, C, nc.EPS, nc.DECAY, ptr(ws), ws.numel(), sp()),
               lib.mrcnn_bn_train_bwd_pair_f32(ptr(x), ptr(x), ptr(x), ptr(x), ptr(v[0]), ptr(v[0]), ptr(v[1]), ptr(v[0]), ptr(v[0]), ptr(v[1]), ptr(out),
                                               ptr(out2), ptr(v[2]), ptr(v[3]), ptr(v[4]), ptr(v[5]), P, C, ptr(ws), ws.numel(), sp())]
        for rc in rcs:
            assert rc == -1 and b'multiple of 256' in lib.mrcnn_last_error()        # MRCNN_E_INVALID
        torch.cuda.synchronize()
        assert all(float(t.min()) == 7.0 == float(t.max()) for t in v[2:6] + [out, out2])
        with pytest.raises(_hip.MrcnnHipError, match='multiple of 256'):
            ops.bn_train_fwd(x, v[0], v[1])
        # fed by partial rows there is no reduction pass: the count is taken
        part = torch.zeros((1, 2, C), device=DEV)
        part[0, 0] = P
        part[0, 1] = P
        o, m, s = ops.bn_train_fwd_stats(x, part, v[0], v[1])
        assert float(m.min()) == 1.0 == float(m.max()) and torch.equal(o, v[1].expand(P, C))


# ---- the layer kernels: one trip past the grid (4096 blocks x 256 threads = 1,048,576 float4 groups), and a small ragged shape ----------
BIG = (1, 129, 128, 256)         # 1,056,768 float4 groups, odd H
BIG_IN = (1, 257, 256, 256)      # its 2x2 / 2 pooling input: odd H and the cover_all row


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('shape', [BIG_IN, (2, 7, 5, 8)], ids=['wraps', 'ragged'])
def test_maxpool_forward_and_backward(shape):
    x = _rand(shape, 1)
    x.requires_grad_(True)
    y = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    gy = _rand(tuple(y.shape), 2)
    y.backward(gy)
    xd = x.detach().to(DEV)
    yd = ops.maxpool2x2_fwd(xd)
    if shape == BIG_IN:
        assert tuple(yd.shape) == BIG
    np.testing.assert_array_equal(_n(yd), _n(y))
    np.testing.assert_array_equal(_n(ops.maxpool2x2_bwd(xd, gy.contiguous().to(DEV))), _n(x.grad))


@pytest.mark.parametrize('shape', [(1, 259, 257, 256), (2, 8, 5, 8)], ids=['wraps', 'ragged'])
def test_maxpool3x3s2_forward(shape):
    x = _rand(shape, 3)
    y = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1)
    yd = ops.maxpool3x3s2_fwd(x.to(DEV))
    if shape[1] == 259:
        assert tuple(yd.shape) == BIG
    np.testing.assert_array_equal(_n(yd), _n(y))


@pytest.mark.parametrize('shape', [BIG, (2, 7, 9, 8)], ids=['wraps', 'ragged'])
def test_upsample_add_forward(shape):
    N, H, W, C = shape
    top, lat = _rand((N, (H + 1) // 2, (W + 1) // 2, C), 4), _rand(shape, 5)
    want = top.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W] + lat
    np.testing.assert_array_equal(_n(ops.upsample2x_add_fwd(top.to(DEV), lat.to(DEV))), _n(want))


@pytest.mark.parametrize('shape', [BIG_IN, (2, 7, 9, 8)], ids=['wraps', 'ragged'])
@pytest.mark.parametrize('accumulate', [False, True], ids=['overwrite', 'accumulate'])
def test_upsample_backward(shape, accumulate):
    """gtop (+)= the in-bounds 2x2 block of gout, added in the kernel's order (dy, dx row-major, after the accumulated value): float32
    additions in that order on the CPU are the same bits."""
    N, H, W, C = shape
    Ht, Wt = (H + 1) // 2, (W + 1) // 2
    gout = _rand(shape, 6)
    base = _rand((N, Ht, Wt, C), 7)
    pad = torch.zeros((N, 2 * Ht, 2 * Wt, C))
    pad[:, :H, :W] = gout
    want = base.clone() if accumulate else torch.zeros_like(base)
    for dy in range(2):
        for dx in range(2):
            want = want + pad[:, dy::2, dx::2]          # an out-of-bounds cell adds +0: the same bits (no -0 sums arise from randn)
    if accumulate:
        got = ops.upsample2x_bwd(gout.to(DEV), gtop=base.clone().to(DEV))
    else:
        got = ops.upsample2x_bwd(gout.to(DEV), top_shape=(N, Ht, Wt, C))
    if shape == BIG_IN:
        assert tuple(got.shape) == BIG
    np.testing.assert_array_equal(_n(got), _n(want))


@pytest.mark.parametrize('shape,stride', [(BIG, 2), (BIG, 1), ((2, 7, 9, 8), 2), ((2, 5, 6, 8), 1)], ids=['wraps_s2', 'wraps_s1', 'ragged_s2', 'ragged_s1'])
@pytest.mark.parametrize('accumulate', [False, True], ids=['overwrite', 'accumulate'])
def test_subsample_backward(shape, stride, accumulate):
    """gx = gsub scattered to the stride lattice (zeros elsewhere), or added into gx there; with relu_x the lattice positions are zeroed
    where relu_x <= 0 and, when accumulating, positions off the lattice keep what gx held."""
    N, H, W, C = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gsub, relu_x, base = _rand((N, Ho, Wo, C), 8), _rand(shape, 9), _rand(shape, 10)
    for with_relu in (False, True):
        want = base.clone() if accumulate else torch.zeros(shape)
        lat = want[:, ::stride, ::stride] + gsub if accumulate else gsub.clone()
        if with_relu:
            lat = torch.where(relu_x[:, ::stride, ::stride] > 0, lat, torch.zeros_like(lat))
        want[:, ::stride, ::stride] = lat
        got = ops.subsample_bwd(gsub.to(DEV), shape, stride, gx=base.clone().to(DEV) if accumulate else None,
                                relu_x=relu_x.to(DEV) if with_relu else None)
        np.testing.assert_array_equal(_n(got), _n(want))


@pytest.mark.parametrize('shape', [(1, 65, 64, 256), (2, 3, 5, 8)], ids=['wraps', 'ragged'])
def test_pixel_shuffle_both_directions(shape):
    N, H, W, C = shape
    t = _rand((N, H, W, 4 * C), 11)
    b = _rand((C,), 12)
    want = t.reshape(N, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C)
    if H == 65:
        assert want.numel() // 4 > 1048576
    got = ops.pixel_shuffle2x(t.to(DEV))
    np.testing.assert_array_equal(_n(got), _n(want))
    np.testing.assert_array_equal(_n(ops.pixel_shuffle2x(t.to(DEV), bias=b.to(DEV))), _n(want + b))
    np.testing.assert_array_equal(_n(ops.pixel_shuffle2x(got, inverse=True)), _n(t))


@pytest.mark.parametrize('shape', [(1, 65, 64, 256), (2, 7, 5, 8)], ids=['wraps', 'ragged'])
def test_bilinear2x_forward(shape):
    """Four products added: within 4 eps32 sum |w x| of float64 (the weights' two roundings, the product's, the additions')."""
    x = _rand(shape, 13)
    up = lambda t: F.interpolate(t.double().permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=True).permute(0, 2, 3, 1)
    want, bound = up(x), 4 * EPS32 * up(x.abs())
    got = ops.bilinear2x_fwd(x.to(DEV))
    if shape[1] == 65:
        assert got.numel() // 4 > 1048576
    err = (got.cpu().double() - want).abs()
    print('bilinear2x_fwd %s: worst err / bound %.3f' % (shape, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('shape', [BIG, (2, 7, 5, 8)], ids=['wraps', 'ragged'])
def test_bilinear2x_backward(shape):
    """The adjoint gathers up to 3 x 3 weighted output cells per input cell: within 4 eps32 sum |w gy| of float64."""
    N, H, W, C = shape
    gy = _rand((N, 2 * H, 2 * W, C), 14)

    def adjoint(g):
        x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        y = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=True).permute(0, 2, 3, 1)
        y.backward(g.double())
        return x.grad

    want, bound = adjoint(gy), 4 * EPS32 * adjoint(gy.abs())
    got = ops.bilinear2x_bwd(gy.to(DEV))
    err = (got.cpu().double() - want).abs()
    print('bilinear2x_bwd %s: worst err / bound %.3f' % (shape, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('n', [4 * 1056768 + 4, 1000], ids=['wraps', 'ragged'])
def test_relu_forward_backward_and_add(n):
    a, b = _rand((n,), 15), _rand((n,), 16)
    np.testing.assert_array_equal(_n(ops.relu(a.to(DEV))), _n(a.clamp_min(0)))
    y = a.clamp_min(0)
    np.testing.assert_array_equal(_n(ops.relu_bwd(b.to(DEV), y.to(DEV))), _n(torch.where(y > 0, b, torch.zeros_like(b))))
    np.testing.assert_array_equal(_n(ops.add(a.to(DEV), b.to(DEV))), _n(a + b))


@pytest.mark.parametrize('shape', [BIG, (2, 7, 5, 8)], ids=['wraps', 'ragged'])
@pytest.mark.parametrize('relu,res', [(False, False), (True, True)])
def test_bn_infer(shape, relu, res):
    C = shape[-1]
    x, r = _rand(shape, 17) * 2 + 3, _rand(shape, 18)
    gamma, beta, mean, var = _rand((C,), 19) * 0.3 + 1, _rand((C,), 20), _rand((C,), 21) + 3, torch.rand((C,), generator=torch.Generator().manual_seed(22)) + 0.5
    want = gamma.double() * ((x.double() - mean.double()) / torch.sqrt(var.double() + nc.EPS)) + beta.double()
    if res:
        want = want + r.double()
    if relu:
        want = want.clamp_min(0)
    got = ops.bn_infer_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), mean.to(DEV), var.to(DEV), r.to(DEV) if res else None, relu)
    e = _err(got, want.numpy())
    print('bn_infer %s relu %d res %d: err %.3e' % (shape, relu, res, e))
    assert e <= 1e-5


@pytest.mark.parametrize('shape', [(2049, 3, 1, 2048), (3, 5, 7, 8)], ids=['wraps', 'ragged'])
def test_global_average_pool(shape):
    """P values added in order, one division: within (P + 1) eps32 sum |x| / P of float64 (P - 1 additions and the division, each at
    most half an ulp of a value bounded by the sum of magnitudes)."""
    R, H, W, C = shape
    P = H * W
    x = _rand(shape, 23)
    if R == 2049:
        assert R * C // 4 > 1048576
    want = x.double().reshape(R, P, C).mean(1)
    bound = (P + 1) * EPS32 * x.double().abs().reshape(R, P, C).sum(1) / P
    got = ops.global_avg_pool(x.to(DEV))
    err = (got.cpu().double() - want).abs()
    print('global_avg_pool %s: worst err / bound %.3f' % (shape, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
