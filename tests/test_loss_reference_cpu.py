"""Pins tests/loss_reference.py, the float64 restatement the GPU loss tests compare with: against float64 torch (autograd for the
gradients) within a few float64 ulps, against oracle/losses.py within that file's float32 noise, and by hand."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as ol
from tests import loss_reference as ref
from tests.loss_judge import EPS32, ratio

EPS64 = float(np.finfo(np.float64).eps)
ULPS = 32 * EPS64       # "a few ulps": sums of up to 81 exponentials and of thousands of per-row terms, in either order


def _ulps(got, want, floor=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= ULPS * np.maximum(np.abs(want), floor)), np.abs(got - want).max()


def _softmax_inputs(seed, M, K, ignore=-1):
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((M, K)) * 3).astype(np.float32)
    t = rs.randint(0, K, M).astype(np.int32)
    t[rs.rand(M) < 0.3] = ignore
    return x, t


@pytest.mark.parametrize('M,K,ignore', [(1, 1, -1), (257, 2, -1), (100, 8, 7), (37, 81, -1), (5, 3136, -1)])
def test_softmax_cross_entropy_against_torch_and_the_float32_oracle(M, K, ignore):
    x, t = _softmax_inputs(M + K, M, K, ignore)
    if ignore == 7:
        t[t == -1] = 7
    loss, count, g = ref.softmax_cross_entropy(x, t, ignore)
    assert count == max(int((t != ignore).sum()), 1) and g.dtype == np.float64 and loss.dtype == np.float64
    xt = torch.from_numpy(x).double().requires_grad_(True)
    lt = F.cross_entropy(xt, torch.from_numpy(t).long(), ignore_index=ignore, reduction='sum') / max(count, 1)
    lt.backward()
    _ulps(loss, lt.item())
    _ulps(g, xt.grad.numpy(), floor=1.0 / count)            # at the target column p - 1 cancels: absolute in units of 1/count
    lo, go = ol.softmax_cross_entropy(x, t, ignore)
    # |log p| <= 40 on these inputs, so one float32 rounding of log p moves p by up to 20 eps32 of itself; the oracle rounds z, the sum,
    # its log and the difference, then exp and the division: 64 eps32 of max(p, 1) / count per element, and of the loss
    assert abs(float(lo) - loss) <= 64 * EPS32 * abs(loss)
    assert ratio(go, g, 1.0 / count) <= 64 * EPS32


@pytest.mark.parametrize('n', [1, 1000, 16385])
def test_sigmoid_cross_entropy_against_torch_and_the_float32_oracle(n):
    rs = np.random.RandomState(n)
    x = (rs.standard_normal(n) * 2).astype(np.float32)
    if n >= 50:                                     # (torch's log(1 + exp(-100)) is 0, not 3.7e-44: no ramp where that is the whole sum)
        x[:50] = np.linspace(-100, 100, 50, dtype=np.float32)
    t = rs.randint(-1, 2, n).astype(np.int32)
    loss, count, g = ref.sigmoid_cross_entropy(x, t)
    valid = t != -1
    assert count == max(int(valid.sum()), 1)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    sel = torch.from_numpy(valid)
    lt = F.binary_cross_entropy_with_logits(xt[sel], torch.from_numpy(t)[sel].double(), reduction='sum') / count
    lt.backward()
    _ulps(loss, lt.item())
    _ulps(g, xt.grad.numpy(), floor=1.0 / count)
    assert np.all(g[~valid] == 0)
    with np.errstate(over='ignore'):
        lo, go = ol.sigmoid_cross_entropy(x, t)
    assert abs(float(lo) - loss) <= 64 * EPS32 * abs(loss)
    assert ratio(go, g, 1.0 / count) <= 16 * EPS32          # sigmoid - t: relative to 1 / count


@pytest.mark.parametrize('sigma', [1.0, 3.0])
def test_fast_rcnn_loc_loss_against_torch_and_the_float32_oracle(sigma):
    rs = np.random.RandomState(int(sigma))
    M = 500
    x = rs.standard_normal((M, 4)).astype(np.float32)
    t = rs.standard_normal((M, 4)).astype(np.float32)
    label = rs.randint(-1, 3, M).astype(np.int32)
    x[:7] = t[:7]
    loss, count, g = ref.fast_rcnn_loc_loss(x, t, label, sigma)
    assert count == int((label >= 0).sum())
    w = torch.from_numpy((label > 0).astype(np.float64))[:, None]
    xt = torch.from_numpy(x).double().requires_grad_(True)
    lt = F.smooth_l1_loss(w * xt, w * torch.from_numpy(t).double(), beta=1.0 / sigma ** 2, reduction='sum') / count
    lt.backward()
    _ulps(loss, lt.item())
    _ulps(g, xt.grad.numpy())
    assert np.all(g[:7] == 0) and np.all(g[label <= 0] == 0)
    lo, go = ol.fast_rcnn_loc_loss(x, t, label, sigma)
    assert abs(float(lo) - loss) <= 64 * EPS32 * abs(loss)
    assert ratio(go, g) <= 16 * EPS32


def test_calc_mask_loss_is_select_plus_sigmoid_and_matches_the_float32_oracle():
    rs = np.random.RandomState(3)
    R, S, C, n_pos = 9, 7, 5, 4
    x = (rs.standard_normal((R, C, S, S)) * 2).astype(np.float32)
    label = np.zeros(R, np.int32)
    label[:n_pos] = rs.randint(1, C + 1, n_pos)
    gt = rs.randint(0, 2, (n_pos, S, S)).astype(np.int32)
    loss, count, g = ref.calc_mask_loss(x, gt, label)
    assert count == n_pos * S * S and g.shape == x.shape
    xt = torch.from_numpy(x).double().requires_grad_(True)
    sel = xt[torch.arange(n_pos), torch.from_numpy(label[:n_pos]).long() - 1]
    lt = F.binary_cross_entropy_with_logits(sel, torch.from_numpy(gt).double(), reduction='sum') / count
    lt.backward()
    _ulps(loss, lt.item())
    _ulps(g, xt.grad.numpy(), floor=1.0 / count)
    lo, go = ol.calc_mask_loss(x, gt, label)
    assert abs(float(lo) - loss) <= 64 * EPS32 * abs(loss)
    assert ratio(go, g, 1.0 / count) <= 16 * EPS32
    # interleaved rows, ignored pixels inside a positive row: only the counted pixels of the positive rows enter
    label2 = np.array([0, 2, -1, 5, 0, 1, 0, -1, 3], np.int32)
    gt2 = rs.randint(-1, 2, (R, S, S)).astype(np.int32)
    loss2, count2, g2 = ref.calc_mask_loss(x, gt2, label2)
    pos = np.nonzero(label2 > 0)[0]
    assert count2 == int((gt2[pos] != -1).sum())
    want = 0.0
    for r in pos:
        l1, c1, g1 = ref.sigmoid_cross_entropy(x[r, label2[r] - 1], gt2[r])
        want += l1 * c1
        np.testing.assert_allclose(g2[r, label2[r] - 1] * count2, g1 * c1, rtol=ULPS, atol=0)
    _ulps(loss2, want / count2)
    assert np.count_nonzero(g2) == count2


def test_all_rows_ignored_and_one_row_by_hand():
    x = np.array([[1.0, -2.0, 0.5], [0.0, 3.0, 3.0]])
    loss, count, g = ref.softmax_cross_entropy(x, [-1, -1])
    assert loss == 0 and count == 1 and not g.any()
    loss, count, g = ref.softmax_cross_entropy(x, [5, 5], ignore_label=5)
    assert loss == 0 and count == 1 and not g.any()
    loss, count, g = ref.sigmoid_cross_entropy(x, np.full((2, 3), -1))
    assert loss == 0 and count == 1 and not g.any()
    loss, count, g = ref.fast_rcnn_loc_loss(np.ones((2, 4)), np.zeros((2, 4)), [-1, -1], 1.0)
    assert loss == 0 and count == 1 and not g.any()
    # one row, two equal logits, target 0: loss = ln 2, gradient = (1/2 - 1, 1/2)
    loss, count, g = ref.softmax_cross_entropy([[0.0, 0.0]], [0])
    assert abs(loss - np.log(2.0)) <= EPS64 and count == 1
    np.testing.assert_array_equal(g, [[-0.5, 0.5]])
    # the ignore label is a parameter: with ignore_label = 7 a label of 1 counts
    loss, count, g = ref.softmax_cross_entropy([[0.0, np.log(3.0)], [9.0, 9.0]], [1, 7], ignore_label=7)
    assert abs(loss - np.log(4.0 / 3.0)) <= 2 * EPS64 and count == 1
    np.testing.assert_allclose(g, [[0.25, -0.25], [0.0, 0.0]], rtol=4 * EPS64)
    # x = 0: sigmoid = 1/2, loss ln 2 whatever the target; x = ln 3, t = 1: loss ln(4/3), gradient 3/4 - 1
    loss, count, g = ref.sigmoid_cross_entropy([0.0, np.log(3.0), 5.0], [0, 1, -1])
    assert count == 2 and abs(loss - (np.log(2.0) + np.log(4.0 / 3.0)) / 2) <= 2 * EPS64
    np.testing.assert_allclose(g, [0.25, -0.125, 0.0], rtol=4 * EPS64)
    # sigma = 2: |d| = 0.1 < 1/4 is quadratic (4/2 * 0.01, gradient 4 * 0.1), |d| = 1 is linear (1 - 1/8, gradient sign); label 0 rows
    # count in the normaliser and carry no weight
    loss, count, g = ref.fast_rcnn_loc_loss([[0.1, -1.0, 0.0, 0.0], [7.0, 7.0, 7.0, 7.0]], np.zeros((2, 4)), [3, 0], 2.0)
    assert count == 2 and abs(loss - (0.02 + 0.875) / 2) <= 2 * EPS64
    np.testing.assert_allclose(g, [[0.2, -0.5, 0.0, 0.0], [0.0] * 4], rtol=4 * EPS64)


def test_select_channel_and_layouts_by_hand():
    x = np.arange(2 * 3 * 2, dtype=np.float64).reshape(2, 3, 2)
    np.testing.assert_array_equal(ref.select_channel(x, [-1, 0]), [[4, 5], [6, 7]])
    np.testing.assert_array_equal(ref.select_channel(x, [-3, 2]), [[0, 1], [10, 11]])
    gx = ref.select_channel_backward(np.array([[1.0, 2.0], [3.0, 4.0]]), [-1, 1], 3)
    np.testing.assert_array_equal(gx, [[[0, 0], [0, 0], [1, 2]], [[0, 0], [3, 4], [0, 0]]])
    h = np.arange(1 * 2 * 4, dtype=np.float64).reshape(1, 2, 4)             # (R, HW, Cp), C = 3
    y = ref.nhwc_to_nchw(h, 3)
    np.testing.assert_array_equal(y, [[[0, 4], [1, 5], [2, 6]]])
    np.testing.assert_array_equal(ref.nchw_to_nhwc_padded(y, 4), [[[0, 1, 2, 0], [4, 5, 6, 0]]])
    assert ref.nhwc_to_nchw(np.zeros((3, 5, 6, 8)), 7).shape == (3, 7, 5, 6)
    assert ref.nchw_to_nhwc_padded(np.zeros((3, 7, 5, 6)), 8).shape == (3, 5, 6, 8)


def _splitmix64_ints(seed, n):
    """splitmix64 in Python integers: output i (1-based) of the stream whose state starts at seed."""
    m, out = 2 ** 64 - 1, []
    for i in range(1, n + 1):
        z = (seed + 0x9E3779B97F4A7C15 * i) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        out.append((z ^ (z >> 31)) >> 32)
    return np.array(out, np.uint32)


def test_splitmix_keys_seed_zero_and_wrap():
    # the published first outputs of splitmix64 from state 0: E220A8397B1DCDAF 6E789E6AA1B965F4 06C45D188009454F
    np.testing.assert_array_equal(ref.splitmix_keys(0, 3), np.array([0xE220A839, 0x6E789E6A, 0x06C45D18], np.uint32))
    assert ref.splitmix_keys(0, 0).shape == (0,) and ref.splitmix_keys(0, 5).dtype == np.uint32
    for seed in (0, 12345, 2 ** 63 - 1, 2 ** 64 - 1, (2 ** 63 - 1 + 2 * ref.SEED_ADVANCE) % 2 ** 64):
        np.testing.assert_array_equal(ref.splitmix_keys(seed, 300), _splitmix64_ints(seed, 300))
    np.testing.assert_array_equal(ref.splitmix_keys(2 ** 64 + 5, 4), ref.splitmix_keys(5, 4))


def test_softmax2_by_hand():
    p = ref.softmax2([[0.0, 0.0], [0.0, np.log(3.0)], [90.0, -90.0], [-90.0, 90.0], [700.0, 700.0]])
    np.testing.assert_allclose(p[:2], [[0.5, 0.5], [0.25, 0.75]], rtol=4 * EPS64)
    assert p[2, 0] == 1.0 and 0 < p[2, 1] < 1e-78 and p[3, 1] == 1.0 and 0 < p[3, 0] < 1e-78
    np.testing.assert_array_equal(p[4], [0.5, 0.5])
    x = np.random.RandomState(0).standard_normal((50, 2)) * 5
    np.testing.assert_allclose(ref.softmax2(x), torch.softmax(torch.from_numpy(x), -1).numpy(), rtol=ULPS)
