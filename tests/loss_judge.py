"""How a float32 loss kernel's output is judged against the float64 restatement (tests/loss_reference.py); shared by
tests/test_loss_gpu.py and tests/test_rpn_gpu.py.

  * loss value: |got - want| <= 1e-5 * max(|want|, 1e-6) (the project's bar, against a float64 reference);
  * gradients element by element: |got - want| <= rtol * (|want| + extra) + FLT_MIN.  FLT_MIN because a flushed denormal is no error;
    ``extra`` is 1/count at the elements where a one-hot or a target was subtracted (the subtraction cancels relative accuracy: the
    error there is relative to the probability, which is up to 1, times 1/count) and 0 elsewhere;
  * rtol is not chosen in advance: it is 4 x the same elementwise ratio of the float32 NumPy oracle (oracle/losses.py) on the same
    inputs, and at least 16 eps32.  The factor 4 is for the device's expf / logf / log1pf being a few ulps from NumPy's and for the
    kernels' summation order (the online softmax of k_sce_chan included).

A helper of the tests, not a test and not part of the product."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)


def ratio(got, want, extra=0.0):
    """The smallest rtol with |got - want| <= rtol * (|want| + extra) + FLT_MIN everywhere (inf where that takes an error on an
    exact zero, NaN where got has one)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        raise ValueError('shapes differ: %s, %s' % (got.shape, want.shape))
    if not got.size:
        return 0.0
    over = np.maximum(np.abs(got - want) - FLT_MIN, 0.0)
    den = np.abs(want) + extra
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(over == 0, 0.0, over / den)
    return float(np.max(r))


def rtol_from(oracle_got, want, extra=0.0):
    return 4.0 * max(ratio(oracle_got, want, extra), 4.0 * EPS32)


def loss_close(got, want):
    got, want = float(got), float(want)
    assert abs(got - want) <= 1e-5 * max(abs(want), 1e-6), (got, want)


def onehot_extra(shape, t, ignore_label, count):
    """1/count at (r, t[r]) of every counted row of an (M,K) gradient, 0 elsewhere."""
    extra = np.zeros(shape, np.float64)
    t = np.asarray(t, np.int64)
    rows = np.nonzero(t != ignore_label)[0]
    extra[rows, t[rows]] = 1.0 / count
    return extra
