"""The case table of tests/nn_cases.py reaches the edges it names (by the restated reduction plan of csrc/nn.hip), and its float64
references are right: the backward equals torch's float64 autograd, the hand-made partials sum to the float64 sums."""
import numpy as np
import pytest
import torch

from tests import nn_cases as nc


def _has_edge(case, edge):
    G, RPI, nblk, rpb = nc.red_plan(case.P, case.C, case.red_cap)
    blocks = nc.block_rows(case.P, case.C, case.red_cap)
    if edge == 'P<RPI':
        return case.P < RPI
    if edge == 'single_row_tail':
        return nblk > 1 and blocks[-1] == 1
    if edge == 'cap_binds':
        want = (case.P * (case.C // 4) + 4095) // 4096
        return want > case.red_cap and nblk != nc.red_plan(case.P, case.C)[2]
    kind, v = edge
    if kind == 'rows':
        return v in nc.thread_rows(case.P, case.C, case.red_cap)
    if kind == 'nblk':
        return nblk == v
    if kind == 'P':
        return case.P == v
    raise AssertionError(edge)


@pytest.mark.parametrize('case', nc.PLAN_CASES, ids=lambda c: c.name)
def test_every_plan_case_reaches_the_edge_it_names(case):
    assert case.edges
    for e in case.edges:
        assert _has_edge(case, e), (case, e, nc.red_plan(case.P, case.C, case.red_cap), sorted(nc.thread_rows(case.P, case.C, case.red_cap)))
    G, RPI, nblk, rpb = nc.red_plan(case.P, case.C, case.red_cap)
    assert G * RPI == nc.NT and rpb % RPI == 0 and (nblk - 1) * rpb < case.P <= nblk * rpb and 1 <= nblk <= case.red_cap
    assert not nc.channels_refused(case.C)
    assert case.P * case.C <= 2 ** 19 or any(e[0] == 'nblk' and e[1] >= 63 for e in case.edges if isinstance(e, tuple))


def test_the_table_covers_the_row_counts_and_block_counts():
    """Per channel count, the rows one thread sums take every value of the statistics pass's (four in flight + tail) and the backward
    passes' (two in flight + tail) lists - with RPI = 1 (C >= 1024) a thread never has 0 rows -, and the block counts sit on both sides
    of the finaliser's 64 and 256 slices.  The lists are reached, not exceeded by design: natural plans also give other counts."""
    assert len(nc.PLAN_CASES) <= 50
    for C in nc.PLAN_C:
        got = set()
        for c in nc.PLAN_CASES:
            if c.C == C:
                got |= nc.thread_rows(c.P, c.C, c.red_cap)
        need = set(nc.STATS_ROWS) | set(nc.BWD_ROWS)
        if C >= 1024:
            need.discard(0)
        assert need <= got, (C, sorted(need - got))
    named = {e[1] for c in nc.PLAN_CASES for e in c.edges if isinstance(e, tuple) and e[0] == 'rows'}
    assert named == set(nc.STATS_ROWS) | set(nc.BWD_ROWS)
    nblk = {nc.red_plan(c.P, c.C, c.red_cap)[2] for c in nc.PLAN_CASES}
    assert set(nc.NBLK) <= nblk
    assert {e[1] for c in nc.PLAN_CASES for e in c.edges if isinstance(e, tuple) and e[0] == 'nblk'} == set(nc.NBLK) | {3}
    assert {c.P for c in nc.PLAN_CASES} >= {1, 2, 3}
    assert any(c.red_cap == 3 and 'cap_binds' in c.edges for c in nc.PLAN_CASES)
    assert {r for r, _ in nc.PARTIAL_CASES} == {1, 63, 64, 65, 255, 256, 257, 1024} and {C for _, C in nc.PARTIAL_CASES} == {4, 8, 20, 64}
    assert {P for P, _, _, _ in nc.RECOMPUTE_CASES} == {1, 15, 16, 17, 127, 128, 129, 1000}
    assert {r for _, r, _, _ in nc.RECOMPUTE_CASES} == {20.0, 80.0, 400.0} and any(o for _, _, _, o in nc.RECOMPUTE_CASES)


def test_the_restated_plan_on_the_shapes_of_the_step():
    # res2 at 2 x 256 x 256: capped at 1024 blocks; (1, 129, 128, 256): 258 wanted
    assert nc.red_plan(2 * 256 * 256, 256)[2:] == (1024, 128)
    assert nc.red_plan(129 * 128, 256) == (64, 4, 258, 64)
    assert nc.channels_refused(1028) and nc.channels_refused(1536) and not nc.channels_refused(2048) and not nc.channels_refused(1020)


@pytest.mark.parametrize('idx', [3, 19, 36])
def test_float64_backward_equals_autograd(idx):
    case = nc.PLAN_CASES[idx]
    d = nc.plan_data(case)
    for relu, res in ((False, False), (True, False), (True, True)):
        x = torch.from_numpy(d['x']).double().requires_grad_(True)
        gamma = torch.from_numpy(d['gamma']).double().requires_grad_(True)
        beta = torch.from_numpy(d['beta']).double().requires_grad_(True)
        r = torch.from_numpy(d['res']).double().requires_grad_(True)
        from oracle.model import bn_train
        y = bn_train(x, gamma, beta)
        if res:
            y = y + r
        if relu:
            y = y.clamp_min(0)
        y.backward(torch.from_numpy(d['gy']).double())
        yr, mean, var, invstd = nc.bn_forward(d['x'], d['gamma'], d['beta'], d['res'] if res else None, relu)
        np.testing.assert_allclose(yr, y.detach().numpy(), rtol=1e-12, atol=1e-12)
        gx, dz, gg, gb = nc.bn_backward(d['gy'], d['x'], d['gamma'], mean, invstd, yr if relu else None)
        scale = float(x.grad.abs().max())
        np.testing.assert_allclose(gx, x.grad.numpy(), rtol=0, atol=1e-11 * max(scale, 1.0))
        np.testing.assert_allclose(gg, gamma.grad.numpy(), rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(gb, beta.grad.numpy(), rtol=1e-11, atol=1e-11)
        if res:
            np.testing.assert_array_equal(dz, r.grad.numpy())
    # the pair: relu(BN_a(xa) + BN_b(xb))
    xa = torch.from_numpy(d['x']).double().requires_grad_(True)
    xb = torch.from_numpy(d['xb']).double().requires_grad_(True)
    pa = [torch.from_numpy(d[k]).double().requires_grad_(True) for k in ('gamma', 'beta', 'gamma_b', 'beta_b')]
    y = (bn_train(xa, pa[0], pa[1]) + bn_train(xb, pa[2], pa[3])).clamp_min(0)
    y.backward(torch.from_numpy(d['gy']).double())
    yr, (ma, va, sa), (mb, vb, sb) = nc.pair_forward(d['x'], d['gamma'], d['beta'], d['xb'], d['gamma_b'], d['beta_b'])
    np.testing.assert_allclose(yr, y.detach().numpy(), rtol=1e-12, atol=1e-12)
    got = nc.pair_backward(d['gy'], yr, d['x'], d['gamma'], ma, sa, d['xb'], d['gamma_b'], mb, sb)
    for g, w in zip(got, (xa.grad, xb.grad, pa[0].grad, pa[1].grad, pa[2].grad, pa[3].grad)):
        np.testing.assert_allclose(g, w.numpy(), rtol=1e-10, atol=1e-10 * max(1.0, float(w.abs().max())))


def test_float32_restatement_is_the_float64_reference_up_to_rounding():
    case = nc.PLAN_CASES[18]
    d = nc.plan_data(case)
    y32, m32, s32 = nc.bn_forward_f32(d['x'], d['gamma'], d['beta'], d['res'], True)
    y, mean, var, invstd = nc.bn_forward(d['x'], d['gamma'], d['beta'], d['res'], True)
    assert np.abs(y32 - y).max() <= 1e-5 * np.abs(y).max() and np.abs(m32 - mean).max() <= 1e-6 * np.abs(mean).max()
    assert np.abs(s32 - invstd).max() <= 1e-5 * invstd.max()
    gx32, gg32, gb32 = nc.bn_backward_f32(d['gy'], d['x'], d['gamma'], m32, s32, y32)
    gx, _, gg, gb = nc.bn_backward(d['gy'], d['x'], d['gamma'], m32, s32, y32)
    for a, b in ((gx32, gx), (gg32, gg), (gb32, gb)):
        assert np.abs(a - b).max() <= 2e-5 * np.abs(b).max()


@pytest.mark.parametrize('rows,C', nc.PARTIAL_CASES)
def test_hand_made_partials_sum_to_the_float64_sums(rows, C):
    x = (np.random.RandomState(rows + C).standard_normal((nc.PARTIAL_P, C)) * 2 + 3).astype(np.float32)
    part = nc.make_partials(x, rows)
    assert part.shape == (rows, 2, C) and part.dtype == np.float32
    x64 = x.astype(np.float64)
    eps = np.finfo(np.float32).eps
    # each run's float32 sum of n terms is within n * eps of the sum of magnitudes; over the runs: P * eps * sum |.|, far from reached
    np.testing.assert_allclose(part[:, 0].astype(np.float64).sum(0), x64.sum(0), rtol=0, atol=16 * eps * np.abs(x64).sum(0).max())
    np.testing.assert_allclose(part[:, 1].astype(np.float64).sum(0), (x64 * x64).sum(0), rtol=16 * eps)


def test_the_recompute_and_first_row_constructions():
    for P, ratio, C, only_one in nc.RECOMPUTE_CASES:
        x = nc.large_mean_data(P, ratio, C, only_one)
        mean, var, _ = nc.bn_stats(x)
        if P >= 127:
            r = np.abs(mean) / np.sqrt(var)
            big = r > 32
            if only_one:
                assert big.sum() == len(range(5, C, 16)) and big[5::16].all()
            else:
                assert big.all() == (ratio > 32) and (ratio > 32 or not big.any())
    for P, C in nc.FIRST_ROW_SHAPES:
        x, k = nc.first_row_data(P, C)
        rest = x[1:].astype(np.float64)
        sd = rest.std(0)
        assert np.all(x[:, C - 1] == x[0, C - 1]) and abs(sd[C - 2] - 1e-3) < 2e-4 and abs(abs(x[0, C - 2] - rest[:, C - 2].mean()) - 1) < 1e-3
        live = np.arange(C) < C - 2
        off = (x[0].astype(np.float64) - rest.mean(0)) / np.where(sd > 0, sd, 1)
        np.testing.assert_allclose(off[live], k[live], rtol=0.15)
        assert {10.0, 100.0, 1000.0} <= set(np.abs(k[live]))
