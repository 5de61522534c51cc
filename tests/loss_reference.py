"""NumPy float64 restatement of the loss tail of the training step and of the one-launch helpers next to it (csrc/loss.hip,
mrcnn_softmax2_f32, mrcnn_random_keys_dev_u32), written from the rules the kernels replace: Chainer's softmax_cross_entropy /
sigmoid_cross_entropy (normalize=True, an ignore label), ChainerCV's _fast_rcnn_loc_loss, calc_mask_loss (channel select + sigmoid
cross entropy), NumPy's fancy index x[arange(R), idx], the NHWC <-> NCHW layout change and splitmix64.  Every floating-point value is
float64 from the first line to the last, so that a comparison against it shows the error of the thing compared and not its own
(oracle/losses.py states the same rules in the kernels' own precision).  Each loss returns (loss, count, gradient): the mean over the
counted elements, the normaliser max(number counted, 1) and d loss / d x.  Pinned by tests/test_loss_reference_cpu.py.  A helper of the
tests, not a test and not part of the product."""
import numpy as np

D = np.float64


def _count(valid):
    return max(int(np.count_nonzero(valid)), 1)


def softmax_cross_entropy(x, t, ignore_label=-1):
    """x (M,K) logits, t (M,) class indices; rows with t == ignore_label do not count."""
    x = np.asarray(x, D)
    t = np.asarray(t, np.int64)
    rows = np.arange(x.shape[0])
    z = x - x.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    valid = t != ignore_label
    count = _count(valid)
    tt = np.where(valid, t, 0)
    loss = -(logp[rows, tt] * valid).sum() / count
    g = np.exp(logp)
    g[rows, tt] -= 1.0
    return D(loss), count, g * valid[:, None] / count


def _sigmoid(x):
    e = np.exp(-np.abs(x))                      # never overflows
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_cross_entropy(x, t):
    """x logits, t targets in {0, 1, -1} of the same shape; elements with t == -1 do not count."""
    x = np.asarray(x, D)
    t = np.asarray(t, np.int64)
    valid = t != -1
    count = _count(valid)
    tf = t.astype(D)
    per = np.maximum(x, 0.0) - x * tf + np.log1p(np.exp(-np.abs(x)))
    loss = (per * valid).sum() / count
    return D(loss), count, (_sigmoid(x) - tf) * valid / count


def fast_rcnn_loc_loss(x, t, label, sigma):
    """x, t (M,4) predicted and target offsets, label (M,): rows with label > 0 carry weight 1, the normaliser is the number of rows
    with label >= 0."""
    x = np.asarray(x, D)
    t = np.asarray(t, D)
    label = np.asarray(label, np.int64)
    w = (label > 0).astype(D)[:, None]
    count = _count(label >= 0)
    sigma2 = D(sigma) ** 2
    d = w * (x - t)
    ad = np.abs(d)
    quad = ad < 1.0 / sigma2
    per = np.where(quad, 0.5 * sigma2 * d * d, ad - 0.5 / sigma2)
    gd = np.where(quad, sigma2 * d, np.sign(d))
    return D(per.sum() / count), count, gd * w / count


def select_channel(x, idx):
    """x (R,C,...), idx (R,) in [-C, C): x[arange(R), idx] - negative indices wrap as NumPy's do."""
    x = np.asarray(x)
    return x[np.arange(x.shape[0]), np.asarray(idx, np.int64)]


def select_channel_backward(gy, idx, C):
    """The scatter that is select_channel's backward: zeros (R,C,...) with gy at channel idx[r] of row r."""
    gy = np.asarray(gy)
    gx = np.zeros((gy.shape[0], C) + gy.shape[1:], gy.dtype)
    gx[np.arange(gy.shape[0]), np.asarray(idx, np.int64)] = gy
    return gx


def calc_mask_loss(roi_cls_mask, gt_roi_mask, gt_roi_label):
    """roi_cls_mask (R,C,H,W) logits, gt_roi_mask (n,H,W) in {0, 1, -1} for the first n <= R rows, gt_roi_label (R,): channel
    label - 1 of every row (select_channel), sigmoid cross entropy over the pixels of the rows with label > 0 whose target is not -1.
    The gradient has roi_cls_mask's shape."""
    x = np.asarray(roi_cls_mask, D)
    label = np.asarray(gt_roi_label, np.int64)
    gt = np.asarray(gt_roi_mask, np.int64)
    n = gt.shape[0]
    idx = np.where(label > 0, label - 1, 0)
    sel = select_channel(x, idx)[:n]
    tt = np.where((label[:n] > 0)[:, None, None], gt, -1)
    loss, count, g = sigmoid_cross_entropy(sel, tt)
    gsel = np.zeros((x.shape[0],) + x.shape[2:], D)
    gsel[:n] = g
    return loss, count, select_channel_backward(gsel, idx, x.shape[1])


def nhwc_to_nchw(x, C):
    """x (R,...,Cp) channels-last with Cp >= C -> (R,C,...): the first C channels, channel axis moved to the front."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(x)[..., :C], -1, 1))


def nchw_to_nhwc_padded(y, Cp):
    """The inverse: y (R,C,...) -> (R,...,Cp) with the channels C..Cp-1 zero."""
    y = np.asarray(y)
    out = np.zeros((y.shape[0],) + y.shape[2:] + (Cp,), y.dtype)
    out[..., :y.shape[1]] = np.moveaxis(y, 1, -1)
    return out


def splitmix_keys(seed, n):
    """The high 32 bits of splitmix64 outputs 1..n of the stream that starts at state ``seed``, in uint64 arithmetic (mod 2^64)."""
    with np.errstate(over='ignore'):
        z = np.uint64(int(seed) % 2 ** 64) + np.uint64(0x9E3779B97F4A7C15) * np.arange(1, n + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


SEED_ADVANCE = 0xD1B54A32D192ED03          # what one draw from a device seed state adds to it (mod 2^64)


def softmax2(x):
    """x (...,2) -> softmax over the last axis."""
    x = np.asarray(x, D)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)
