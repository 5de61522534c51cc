"""GPU parity tests: fused loss kernels (loss.hip, through the C ABI) against the NumPy oracle
(oracle/losses.py).  Floating point => tolerance 1e-5 relative on the loss, 1e-5 absolute-relative on
gradients (the north-star bar is 1e-3).

Below those, every entry point of loss.hip against the float64 restatement tests/loss_reference.py (pinned on the CPU by
tests/test_loss_reference_cpu.py) at the shapes where each kernel takes another path, judged by tests/loss_judge.py: counts exact,
the loss within 1e-5 of the float64 value, gradients element by element within rtol * (|want| + 1/count where a one-hot or a target
was subtracted) + FLT_MIN with rtol = 4 x max(the float32 oracle's own ratio on the same inputs, 4 eps32), data movement bit for bit,
fully written outputs from NaN-filled buffers.

Observed on an MI355X (largest elementwise gradient ratio over the cases of each kernel, in eps32, against the bound of the case that
gave it; the float32 oracle's own ratio is a quarter of the bound):
  k_sce_small 8.1 of 36.7    k_sce_wave 17.4 of 68.7 (the +-80 logits)    k_sce_chan 57.7 of 231.2 (the -40..40 ramp over 3136
  positions; 17.5 of 65.8 elsewhere)    k_sl1 1.3 of 16    k_mask_bce 0.75 of 16    k_sigmoid_ce 0.72 of 16, 0.82 of 48 through autograd
  with the x3 of k_scale_dev    k_softmax2 (tests/test_rpn_gpu.py) 8.8 of 37.2
No kernel is above the oracle's own ratio by more than rounding.  Loss values: within 8.7e-8 of the float64 value everywhere (bar 1e-5).
"""
import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import loss_reference as ref
from tests.loss_judge import EPS32, loss_close, onehot_extra, ratio, rtol_from

pytestmark = pytest.mark.gpu

from chainer_maskrcnn._hip import check, lib, ops, ptr, stream_ptr  # noqa: E402
from chainer_maskrcnn.functions import loss as fl  # noqa: E402

DEV = 'cuda:0'


def _close(got, want, tol=1e-5):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert np.abs(got - want).max() <= tol * max(np.abs(want).max(), 1e-6), np.abs(got - want).max()


@pytest.mark.parametrize('M,K,ld', [(1000, 2, 2), (37, 81, 96), (5, 3136, 3136), (0, 2, 2), (300000, 2, 2)])
def test_softmax_cross_entropy(M, K, ld):
    rs = np.random.RandomState(M + K)
    x = (rs.standard_normal((M, ld)) * 3).astype(np.float32)
    t = rs.randint(-1, K, M).astype(np.int32)
    loss, g = ol.softmax_cross_entropy(x[:, :K], t) if M else (np.float32(0), np.zeros((0, K), np.float32))
    xd = torch.from_numpy(x).to(DEV)
    out, gx = ops.softmax_ce(xd, torch.from_numpy(t).to(DEV), M, K, (1, ld, 0, 1), Kfill=ld if ld > K else 0)
    out = out.cpu().numpy()
    _close(out[0], loss)
    assert out[1] == max((t != -1).sum(), 1)
    if M:
        _close(gx.cpu().numpy()[:, :K], g)
        assert np.all(gx.cpu().numpy()[:, K:] == 0)


def test_softmax_cross_entropy_all_ignored():
    x = torch.randn((10, 2), device=DEV)
    t = torch.full((10,), -1, dtype=torch.int32, device=DEV)
    out, gx = ops.softmax_ce(x, t, 10, 2, (1, 2, 0, 1))
    assert out[0].item() == 0 and torch.all(gx == 0)


@pytest.mark.parametrize('R,HW,K,Cm', [(3, 49, 17, 32), (5, 3136, 17, 32), (1300, 64, 17, 32), (4, 200, 3, 4), (2, 777, 40, 64), (2, 100, 17, 20)])
def test_softmax_cross_entropy_keypoint_layout(R, HW, K, Cm):
    """rows = (roi, keypoint), elements strided over NHWC positions (train_keypoints.py:21-27): the one-wave-per-row kernel (HW < 64
    or a channel count the coalesced kernel does not take) and the channel-interleaved kernel (one workgroup per RoI, float4 loads
    over the (position, channel) plane, loss partials and gradient from one launch, more RoIs than partial slots); with the
    coalesced kernel the callee writes the WHOLE gradient tensor - zeros in the padded channels and the ignored rows - so a
    NaN-filled buffer must come back finite."""
    rs = np.random.RandomState(HW + K)
    x = (3.0 * rs.standard_normal((R, HW, Cm))).astype(np.float32)
    x[0, HW // 2, 0] = 60.0                                    # a dominant logit: the running maximum moves late
    t = rs.randint(-1, HW, (R, K)).astype(np.int32)
    t[-1] = -1                                                 # a RoI whose rows are all ignored
    logical = x[:, :, :K].transpose(0, 2, 1).reshape(R * K, HW)
    loss, g = ol.softmax_cross_entropy(logical, t.reshape(-1))
    xd = torch.from_numpy(x).to(DEV)
    xmap = (K, HW * Cm, 1, Cm)
    fills = ops.softmax_ce_fills_gradient(R * K, HW, xmap)
    assert fills == (HW >= 64 and Cm in (4, 32, 64))
    gx = torch.full_like(xd, float('nan')) if fills else torch.zeros_like(xd)
    out, gx = ops.softmax_ce(xd, torch.from_numpy(t.reshape(-1)).to(DEV), R * K, HW, xmap, gx=gx)
    _close(out[0].item(), loss)
    assert out[1].item() == max(1, int((t != -1).sum()))
    got = gx.cpu().numpy()
    assert np.isfinite(got).all()
    assert (got[:, :, K:] == 0).all() and (got[-1] == 0).all()
    _close(got[:, :, :K].transpose(0, 2, 1).reshape(R * K, HW), g)
    out2, _ = ops.softmax_ce(xd, torch.from_numpy(t.reshape(-1)).to(DEV), R * K, HW, xmap, want_grad=False)      # loss only
    assert out2[0].item() == out[0].item()


@pytest.mark.parametrize('sigma', [1.0, 3.0])
@pytest.mark.parametrize('M,ld', [(500, 4), (64, 32), (0, 4)])
def test_smooth_l1(sigma, M, ld):
    rs = np.random.RandomState(int(sigma) + M)
    x = rs.standard_normal((M, ld)).astype(np.float32)
    t = rs.standard_normal((M, 4)).astype(np.float32)
    label = rs.randint(-1, 3, M).astype(np.int32)
    if M:
        loss, g = ol.fast_rcnn_loc_loss(x[:, :4], t, label, sigma)
    out, gx = ops.smooth_l1(torch.from_numpy(x).to(DEV), ld, torch.from_numpy(t).to(DEV), torch.from_numpy(label).to(DEV),
                            M, sigma, gfill=ld)
    if M:
        _close(out[0].item(), loss)
        _close(gx.cpu().numpy()[:, :4], g)
        assert np.all(gx.cpu().numpy()[:, 4:] == 0)


def test_mask_bce_matches_calc_mask_loss():
    rs = np.random.RandomState(3)
    R, S, Cm, n_pos, n_cls = 12, 28, 96, 5, 80
    x = rs.standard_normal((R, S, S, Cm)).astype(np.float32) * 2
    label = np.zeros(R, np.int32)
    label[:n_pos] = rs.randint(1, n_cls + 1, n_pos)
    gt = rs.randint(0, 2, (R, S, S)).astype(np.int32)
    gt[n_pos:] = -1
    nchw = x[:, :, :, :n_cls].transpose(0, 3, 1, 2)
    loss, g = ol.calc_mask_loss(nchw, gt[:n_pos], label)
    out, gx = ops.mask_bce(torch.from_numpy(x).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(label).to(DEV))
    _close(out[0].item(), loss)
    assert out[1].item() == n_pos * S * S
    got = gx.cpu().numpy()
    _close(got[:, :, :, :n_cls].transpose(0, 3, 1, 2), g)
    assert np.all(got[:, :, :, n_cls:] == 0)


# ---- every loss.hip entry point against the float64 restatement (tests/loss_reference.py), judged by tests/loss_judge.py ------------
# Shapes: the smallest that cross each boundary.  grid_for caps a launch at 1024 blocks of 256 threads: a one-thread-per-item kernel
# wraps its grid-stride loop above 262144 items, k_sce_wave (one wave per row) above 4096 rows; k_finalize sums nb = min(ceil(n / 256),
# 1024) partials, four per lane per iteration while k + 192 < nb (first at nb = 193) and one per lane in its tail loop.
def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _nan(shape):
    return torch.full(tuple(shape), float('nan'), dtype=torch.float32, device=DEV)


def _loss_ws():
    return torch.empty((lib().mrcnn_loss_workspace_bytes(),), dtype=torch.uint8, device=DEV)


def _judge(kernel, got, want, oracle_got, extra=0.0, factor=1.0):
    """The elementwise gradient bound of tests/loss_judge.py; prints the observed ratio (the module docstring quotes the maxima)."""
    rtol = factor * rtol_from(oracle_got, want, extra)
    r = ratio(got, want, extra)
    print('LOSSRATIO %s %.2f eps32 (bound %.2f eps32)' % (kernel, r / EPS32, rtol / EPS32))
    assert r <= rtol, (kernel, r / EPS32, rtol / EPS32)


def _softmax_check(kernel, logical, t, out, got_logical, ignore=-1):
    """loss, count and the (M,K) gradient of one softmax_ce call against the float64 reference, rtol from the float32 oracle."""
    loss, count, g = ref.softmax_cross_entropy(logical, t, ignore)
    out = out.cpu().numpy()
    print('LOSSVALUE %s rel %.3g' % (kernel, abs(float(out[0]) - loss) / max(abs(loss), 1e-6)))
    loss_close(out[0], loss)
    assert out[1] == count
    extra = onehot_extra(g.shape, t, ignore, count)
    _judge(kernel, got_logical, g, ol.softmax_cross_entropy(logical, t, ignore)[1], extra)
    assert np.all(got_logical[np.asarray(t) == ignore] == 0)


def _labels(rs, M, K, ignore=-1, p_ignore=0.25):
    t = rs.randint(0, K, M).astype(np.int32)
    t[rs.rand(M) < p_ignore] = ignore
    return t


@pytest.mark.parametrize('K', [1, 2, 8])
@pytest.mark.parametrize('M', [1, 255, 257])
def test_softmax_ce_small_path_float64(M, K):
    rs = np.random.RandomState(10 * M + K)
    x = (rs.standard_normal((M, K)) * 3).astype(np.float32)
    t = _labels(rs, M, K)
    if M == 1:
        t[0] = K - 1
    out, gx = ops.softmax_ce(_d(x), _d(t), M, K, (1, K, 0, 1), gx=_nan((M, K)))
    _softmax_check('k_sce_small', x, t, out, gx.cpu().numpy())


def test_softmax_ce_small_path_other_ignore_label():
    """ignore_label = 7: the labels equal to 7 are the ignored ones, -1 does not occur (class 7 is never a target)."""
    rs = np.random.RandomState(7)
    M, K = 257, 8
    x = (rs.standard_normal((M, K)) * 3).astype(np.float32)
    t = rs.randint(0, 8, M).astype(np.int32)
    assert (t == 7).any() and (t != 7).any() and (t >= 0).all()
    out, gx = ops.softmax_ce(_d(x), _d(t), M, K, (1, K, 0, 1), gx=_nan((M, K)), ignore_label=7)
    _softmax_check('k_sce_small', x, t, out, gx.cpu().numpy(), ignore=7)
    assert out[1].item() == (t != 7).sum()


def test_softmax_ce_small_path_head_layout_and_a_dense_gradient_map():
    """Scores read in place from a (P, Cp = 20) head buffer - row (p, a), a < A = 3, class j at p * Cp + 4A + 2a + j - and the gradient
    written through another map, a dense (M, 2): the first A > 1 on this path and the first gmap != xmap."""
    rs = np.random.RandomState(20)
    P, A, Cp = 100, 3, 20
    M = P * A
    head = (rs.standard_normal((P, Cp)) * 3).astype(np.float32)
    t = _labels(rs, M, 2)
    logical = head[:, 4 * A:6 * A].reshape(M, 2)
    hd = _d(head)
    gx = _nan((M, 2))
    out, _ = ops.softmax_ce(hd.view(-1)[4 * A:], _d(t), M, 2, (A, Cp, 2, 1), gmap=(A, 2 * A, 2, 1), gx=gx)
    _softmax_check('k_sce_small', logical, t, out, gx.cpu().numpy())
    np.testing.assert_array_equal(hd.cpu().numpy(), head)


@pytest.mark.parametrize('Kfill', [0, 96])
@pytest.mark.parametrize('K', [9, 63, 64, 65, 81])
@pytest.mark.parametrize('M', [4097, 1])
def test_softmax_ce_wave_path_float64(M, K, Kfill):
    """One wave per row: K below, at and above the wave width, 4097 rows (the grid-stride loop wraps), a gradient buffer wider than K
    whose columns K..Kfill-1 must come back zero from NaN.  The M = 4097, K = 81 case carries logits a naive exp would overflow on."""
    rs = np.random.RandomState(M + K + Kfill)
    ld = Kfill or K
    x = (rs.standard_normal((M, ld)) * 3).astype(np.float32)
    t = _labels(rs, M, K)
    if M == 1:
        t[0] = K - 1
    if M == 4097 and K == 81:
        r7, r11 = np.arange(0, M, 7), np.arange(0, M, 11)
        x[r7, r7 % K] = 80.0
        x[r11, (r11 + 5) % K] = -80.0
        x[4000] = 0.0
    assert not ops.softmax_ce_fills_gradient(M, K, (1, ld, 0, 1), Kfill=Kfill)
    out, gx = ops.softmax_ce(_d(x), _d(t), M, K, (1, ld, 0, 1), Kfill=Kfill, gx=_nan((M, ld)))
    got = gx.cpu().numpy()
    _softmax_check('k_sce_wave', x[:, :K], t, out, got[:, :K])
    assert np.all(got[:, K:] == 0)


def _chan_case(rs, G, K, C, A, x=None):
    x = (rs.standard_normal((G, K, C)) * 3).astype(np.float32) if x is None else x
    t = rs.randint(-1, K, (G, A)).astype(np.int32)
    t[0, 0], t[-1, -1] = 0, K - 1                       # targets at the first and the last position
    if G * A > 2:
        t[G // 2, A // 2] = -1
    return x, t, np.ascontiguousarray(x[:, :, :A].transpose(0, 2, 1)).reshape(G * A, K)


def _chan_run(x, t, K, C, A, want_grad=True):
    G = x.shape[0]
    xmap = (A, K * C, 1, C)
    xd = _d(x)
    fills = ops.softmax_ce_fills_gradient(G * A, K, xmap)
    gx = (_nan(x.shape) if fills else torch.zeros_like(xd)) if want_grad else None
    out, gx = ops.softmax_ce(xd, _d(t.reshape(-1)), G * A, K, xmap, gx=gx, want_grad=want_grad)
    return fills, out, gx


@pytest.mark.parametrize('C,A', [(8, 1), (8, 8), (16, 1), (16, 16), (128, 1), (128, 17), (128, 128), (256, 1), (256, 17), (256, 256)])
@pytest.mark.parametrize('K', [64, 63])
def test_softmax_ce_channel_interleaved_path_float64(K, C, A):
    """k_sce_chan at the channel counts the existing cases leave out (8, 16, 128, 256), with one row, 17 rows and C rows per group, at
    K = 64, the smallest K it takes; K = 63 must not take it (the library's own predicate) and is then the wave kernel on strided rows."""
    rs = np.random.RandomState(K + C + A)
    G = 3
    x, t, logical = _chan_case(rs, G, K, C, A)
    fills, out, gx = _chan_run(x, t, K, C, A)
    assert fills == (K >= 64)
    got = gx.cpu().numpy()
    assert not np.isnan(got).any()
    _softmax_check('k_sce_chan' if fills else 'k_sce_wave', logical, t.reshape(-1), out, got[:, :, :A].transpose(0, 2, 1).reshape(G * A, K))
    assert np.all(got[:, :, A:] == 0)
    _, out2, _ = _chan_run(x, t, K, C, A, want_grad=False)
    assert out2.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()          # the loss-only launch gives the same bits


def test_softmax_ce_channel_interleaved_running_maximum_moves_every_step():
    """Logits that rise from -40 to 40 along the K = 3136 positions: every position a thread visits is a new maximum, so the online
    softmax rescales its sum at every step."""
    rs = np.random.RandomState(5)
    G, K, C, A = 2, 3136, 32, 17
    ramp = np.linspace(-40.0, 40.0, K)
    x = (ramp[None, :, None] + 0.01 * np.arange(C)[None, None, :] + 0.5 * np.arange(G)[:, None, None]).astype(np.float32)
    assert np.all(np.diff(x, axis=1) > 0)
    x, t, logical = _chan_case(rs, G, K, C, A, x)
    t[1, :4] = [K - 1, K - 2, K - 40, K // 2]
    fills, out, gx = _chan_run(x, t, K, C, A)
    assert fills
    got = gx.cpu().numpy()
    _softmax_check('k_sce_chan', logical, t.reshape(-1), out, got[:, :, :A].transpose(0, 2, 1).reshape(G * A, K))
    assert np.all(got[:, :, A:] == 0)


def test_softmax_ce_channel_interleaved_all_rows_ignored():
    rs = np.random.RandomState(6)
    G, K, C, A = 3, 64, 32, 17
    x = (rs.standard_normal((G, K, C)) * 3).astype(np.float32)
    t = np.full((G, A), -1, np.int32)
    fills, out, gx = _chan_run(x, t, K, C, A)
    assert fills
    np.testing.assert_array_equal(out.cpu().numpy(), np.array([0, 1], np.float32))
    assert np.all(gx.cpu().numpy() == 0)


def _sl1_inputs(rs, M):
    x = rs.standard_normal((M, 4)).astype(np.float32)
    t = rs.standard_normal((M, 4)).astype(np.float32)
    label = rs.randint(-1, 3, M).astype(np.int32)
    return x, t, label


def test_smooth_l1_wraps_and_exact_zero_gradients():
    """262145 rows (the grid-stride loop wraps), labels from {-1, 0, 1, 2}, two whole workgroups of rows labelled -1 (their partials
    are (0, 0)), and rows with label > 0 whose prediction equals its target: gradient exactly 0."""
    rs = np.random.RandomState(11)
    M, sigma = 262145, 3.0
    x, t, label = _sl1_inputs(rs, M)
    label[512:1024] = -1
    eq = np.arange(5, M, 1001)
    label[eq] = 1 + (eq % 2)
    x[eq] = t[eq]
    label[-1] = 2                                      # the row only the wrapped iteration reaches counts
    loss, count, g = ref.fast_rcnn_loc_loss(x, t, label, sigma)
    out, gx = ops.smooth_l1(_d(x), 4, _d(t), _d(label), M, sigma, gx=_nan((M, 4)))
    out, got = out.cpu().numpy(), gx.cpu().numpy()
    print('LOSSVALUE k_sl1 rel %.3g' % (abs(float(out[0]) - loss) / abs(loss)))
    loss_close(out[0], loss)
    assert out[1] == count == (label >= 0).sum()
    _judge('k_sl1', got, g, ol.fast_rcnn_loc_loss(x, t, label, sigma)[1])
    assert np.all(got[eq] == 0) and np.all(got[label <= 0] == 0) and np.any(got[-1] != 0)


def test_smooth_l1_column_offset_fill_and_untouched_columns():
    """col0 = 4, ldx = 12, gfill = 8 into a NaN-filled gradient: columns 4..7 receive the gradient, 8..11 zeros, 0..3 stay NaN."""
    rs = np.random.RandomState(12)
    M, sigma = 300, 1.0
    x, t, label = _sl1_inputs(rs, M)
    buf = rs.standard_normal((M, 12)).astype(np.float32)
    buf[:, 4:8] = x
    loss, count, g = ref.fast_rcnn_loc_loss(x, t, label, sigma)
    out, gx = ops.smooth_l1(_d(buf), 12, _d(t), _d(label), M, sigma, gfill=8, col0=4, gx=_nan((M, 12)))
    out, got = out.cpu().numpy(), gx.cpu().numpy()
    loss_close(out[0], loss)
    assert out[1] == count
    _judge('k_sl1', got[:, 4:8], g, ol.fast_rcnn_loc_loss(x, t, label, sigma)[1])
    assert np.all(got[:, 8:] == 0) and np.isnan(got[:, :4]).all()


def test_smooth_l1_all_labels_ignored():
    rs = np.random.RandomState(13)
    M = 700
    x, t, _ = _sl1_inputs(rs, M)
    out, gx = ops.smooth_l1(_d(x), 4, _d(t), _d(np.full(M, -1, np.int32)), M, 3.0, gx=_nan((M, 4)))
    np.testing.assert_array_equal(out.cpu().numpy(), np.array([0, 1], np.float32))        # the count clamps to 1
    assert np.all(gx.cpu().numpy() == 0)


def _ramp_logits():
    return np.linspace(-100.0, 100.0, 50).astype(np.float32)


def test_mask_bce_wraps_interleaved_rows_and_ignored_pixels():
    """340 x 784 = 266560 pixels (the grid-stride loop wraps); positive rows interleaved with rows of label 0 and -1; a third of the
    pixels of every row - the positive ones included - carry gt == -1; one label equals n_cls; logits of scale 2 and a ramp from -100 to
    100 on counted pixels.  The gradient is zero everywhere but the selected channel of the counted pixels (channel Cm - 1 is padding)."""
    rs = np.random.RandomState(14)
    Rm, S, Cm, n_cls = 340, 28, 4, 3
    x = (rs.standard_normal((Rm, S, S, Cm)) * 2).astype(np.float32)
    label = np.where(np.arange(Rm) % 3 == 0, rs.randint(1, n_cls + 1, Rm), np.where(np.arange(Rm) % 3 == 1, 0, -1)).astype(np.int32)
    label[3] = n_cls
    label[-1] = 1                                       # the rows of the wrapped iteration count too
    gt = rs.randint(0, 2, (Rm, S, S)).astype(np.int32)
    gt[rs.rand(Rm, S, S) < 1.0 / 3.0] = -1
    x[0].reshape(-1, Cm)[:50, label[0] - 1] = _ramp_logits()
    gt[0].reshape(-1)[:50] = np.arange(50) % 2
    pos = label > 0
    assert (gt[pos] == -1).mean() > 0.3 and pos[-1] and not pos[1] and not pos[2]
    nchw = ref.nhwc_to_nchw(x, n_cls)
    loss, count, g = ref.calc_mask_loss(nchw, gt, label)
    assert count == (gt[pos] != -1).sum()
    out, gx = ops.mask_bce(_d(x), _d(gt), _d(label))
    out, got = out.cpu().numpy(), gx.cpu().numpy()
    print('LOSSVALUE k_mask_bce rel %.3g' % (abs(float(out[0]) - loss) / abs(loss)))
    loss_close(out[0], loss)
    assert out[1] == count
    counted = pos[:, None, None] & (gt != -1)
    idx = np.where(pos, label - 1, 0)
    sel_mask = ref.select_channel_backward(counted, idx, n_cls)
    assert not np.isnan(got).any() and np.all(got[..., n_cls:] == 0)
    got_nchw = ref.nhwc_to_nchw(got, n_cls)
    assert np.all(got_nchw[~sel_mask] == 0)
    with np.errstate(over='ignore'):
        o_g = ol.sigmoid_cross_entropy(ref.select_channel(nchw, idx), np.where(pos[:, None, None], gt, -1))[1]
    _judge('k_mask_bce', ref.select_channel(got_nchw, idx), ref.select_channel(g, idx), o_g, extra=counted / count)


SIGMOID_N = [0, 1, 16384, 16385, 49153, 65536, 65537, 262145]        # k_finalize at nb = -, 1, 64, 65, 193, 256, 257, 1024 (+ the wrap)


def _sigmoid_inputs(n):
    rs = np.random.RandomState(n)
    x = (rs.standard_normal(n) * 2).astype(np.float32)
    t = rs.randint(-1, 2, n).astype(np.int32)
    if n >= 50:
        x[:50] = _ramp_logits()
        t[:50] = np.arange(50) % 2
    if n:
        t[-1] = 1                                       # the last element (for 262145: the wrapped iteration's) counts
    return x, t


def _sigmoid_lib(x, t):
    n = x.size
    xd, td, out, gx, ws = _d(x), _d(t), _nan((2,)), _nan((n,)), _loss_ws()         # (every device tensor stays referenced over the call)
    check(lib().mrcnn_sigmoid_ce_f32(ptr(xd), ptr(td), n, ptr(out), ptr(gx), ptr(ws), ws.numel(), stream_ptr()))
    return out.cpu().numpy(), gx.cpu().numpy()


@pytest.mark.parametrize('n', SIGMOID_N)
def test_sigmoid_ce_float64_at_every_finalize_block_count(n):
    x, t = _sigmoid_inputs(n)
    loss, count, g = ref.sigmoid_cross_entropy(x, t)
    out, got = _sigmoid_lib(x, t)
    assert out[1] == count
    if n == 0:
        assert out[0] == 0
        return
    print('LOSSVALUE k_sigmoid_ce n=%d rel %.3g' % (n, abs(float(out[0]) - loss) / abs(loss)))
    loss_close(out[0], loss)
    with np.errstate(over='ignore'):
        o_g = ol.sigmoid_cross_entropy(x, t)[1]
    extra = (t != -1) / count
    _judge('k_sigmoid_ce', got, g, o_g, extra)
    assert np.all(got[t == -1] == 0)
    # the autograd function: the same loss bits, and (loss * 3).backward() gives 3 x the gradient (one more rounding: 3 x rtol) -
    # not the unscaled one
    xd = _d(x).requires_grad_(True)
    l = fl.sigmoid_cross_entropy(xd, _d(t))
    assert l.item() == out[0]
    (l * 3).backward()
    got3 = xd.grad.cpu().numpy()
    _judge('k_sigmoid_ce+k_scale_dev', got3, 3 * g, o_g * np.float32(3), 3 * extra, factor=3.0)
    assert ratio(got3, g, extra) > 3 * rtol_from(o_g, g, extra)


def test_sigmoid_ce_all_ignored():
    x, _ = _sigmoid_inputs(1000)
    out, got = _sigmoid_lib(x, np.full(1000, -1, np.int32))
    np.testing.assert_array_equal(out, np.array([0, 1], np.float32))
    assert np.all(got == 0)


def _select_lib(src, idx, R, C, HW, backward):
    sd, ind, dst = _d(src), _d(idx), _nan((R, C, HW) if backward else (R, HW))
    check(lib().mrcnn_select_channel_f32(ptr(sd), ptr(ind), R, C, HW, ptr(dst), int(backward), stream_ptr()))
    return dst.cpu().numpy()


@pytest.mark.parametrize('R,C,HW', [(1, 1, 1), (5, 3, 49), (700, 2, 400), (330, 5, 196)])
def test_select_channel_forward_and_backward_bit_exact(R, C, HW):
    """x[arange(R), idx] with idx in [-C, C) (-1 is channel C - 1, -C is channel 0) and its scatter into a NaN-filled buffer; the
    forward wraps its grid-stride loop at (700, 2, 400), the backward at (330, 5, 196)."""
    rs = np.random.RandomState(R + C + HW)
    x = rs.standard_normal((R, C, HW)).astype(np.float32)
    gy = rs.standard_normal((R, HW)).astype(np.float32)
    idx = rs.randint(-C, C, R).astype(np.int32)
    idx[0] = -1
    idx[-1] = -C
    np.testing.assert_array_equal(_select_lib(x, idx, R, C, HW, False), ref.select_channel(x, idx))
    np.testing.assert_array_equal(_select_lib(gy, idx, R, C, HW, True), ref.select_channel_backward(gy, idx, C))


def test_select_channel_through_mask_logits_autograd():
    rs = np.random.RandomState(15)
    R, C, S = 5, 3, 7
    x = rs.standard_normal((R, C, S, S)).astype(np.float32)
    gy = rs.standard_normal((R, S, S)).astype(np.float32)
    idx = np.array([-1, 0, 2, -3, -2], np.int32)
    leaf = _d(x).requires_grad_(True)
    y = leaf.as_subclass(fl.MaskLogits)[fl.XP(leaf.device).arange(R), _d(idx)]
    np.testing.assert_array_equal(y.detach().cpu().numpy(), ref.select_channel(x, idx))
    y.backward(_d(gy))
    np.testing.assert_array_equal(leaf.grad.cpu().numpy(), ref.select_channel_backward(gy, idx, C))


def _layout_lib(src, R, HW, Cp, C, inverse):
    sd, dst = _d(src), _nan((R, HW, Cp) if inverse else (R, C, HW))
    check(lib().mrcnn_nhwc_nchw_f32(ptr(sd), ptr(dst), R, HW, Cp, C, int(inverse), stream_ptr()))
    return dst.cpu().numpy()


@pytest.mark.parametrize('HW', [1, 31, 32, 33, 784])
def test_nhwc_nchw_tiles_padding_and_inverse_bit_exact(HW):
    """Pixel and channel counts below, at and above the 32 x 32 tile, padded channel counts C, C + 1 and the next multiple of 32, no, one
    and three rows: forward = x[..., :C] transposed, every element written; inverse into a NaN-filled buffer = the zero-padded
    transpose."""
    rs = np.random.RandomState(HW)
    for C in (1, 17, 32, 33, 80):
        for Cp in sorted({C, C + 1, -(-C // 32) * 32}):
            for R in (0, 1, 3):
                x = rs.standard_normal((R, HW, Cp)).astype(np.float32)
                y = rs.standard_normal((R, C, HW)).astype(np.float32)
                np.testing.assert_array_equal(_layout_lib(x, R, HW, Cp, C, False), ref.nhwc_to_nchw(x, C), err_msg=str((C, Cp, R)))
                np.testing.assert_array_equal(_layout_lib(y, R, HW, Cp, C, True), ref.nchw_to_nhwc_padded(y, Cp), err_msg=str((C, Cp, R)))


@pytest.mark.parametrize('R,H,W,Cp,C', [(3, 7, 9, 20, 17), (1, 1, 1, 33, 33), (2, 28, 28, 96, 80)])
def test_nhwc_to_nchw_autograd_pads_the_gradient_back(R, H, W, Cp, C):
    rs = np.random.RandomState(H + W + Cp)
    x = rs.standard_normal((R, H, W, Cp)).astype(np.float32)
    gy = rs.standard_normal((R, C, H, W)).astype(np.float32)
    leaf = _d(x).requires_grad_(True)
    y = fl.nhwc_to_nchw(leaf, C)
    np.testing.assert_array_equal(y.detach().cpu().numpy(), ref.nhwc_to_nchw(x, C))
    y.backward(_d(gy))
    np.testing.assert_array_equal(leaf.grad.cpu().numpy(), ref.nchw_to_nhwc_padded(gy, Cp))


@pytest.mark.parametrize('scale', [0.0, -2.5, 1.0 / 3.0])
@pytest.mark.parametrize('n', [0, 1, 257, 262145])
def test_scale_by_dev_is_the_float32_product(n, scale):
    x = np.random.RandomState(n).standard_normal(n).astype(np.float32)
    want = x * np.float32(scale)
    xd, sd = _d(x), _d(np.array([scale], np.float32))
    check(lib().mrcnn_scale_by_dev_f32(ptr(xd), n, ptr(sd), stream_ptr()))
    np.testing.assert_array_equal(xd.cpu().numpy(), want)
    assert sd.item() == np.float32(scale)


@pytest.mark.parametrize('n', [1, 5])
def test_loss_total_is_the_sequential_sum_of_the_losses_only(n):
    """(loss, normaliser) pairs with distinct normalisers: out = the float32 sum of the losses in order; no normaliser enters."""
    rs = np.random.RandomState(n)
    pairs = np.stack([rs.uniform(0.01, 3.0, n), 100.0 + 17.0 * np.arange(n)], 1).astype(np.float32)
    want = np.float32(0)
    for v in pairs[:, 0]:
        want = np.float32(want + v)
    got = ops.loss_total(_d(pairs)).cpu().numpy()
    np.testing.assert_array_equal(got, np.array([want], np.float32))
