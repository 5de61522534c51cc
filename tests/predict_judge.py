"""How the outputs of the inference post-processing kernels are judged against the float64 restatement (tests/predict_reference.py); shared
by tests/test_predict_gpu.py, tests/test_tta_gpu.py and tests/test_predict_cases_cpu.py.  No tolerance is fixed in advance: each is
loss_judge.rtol_from's rule, 4 x what the float32 NumPy oracle (oracle/predict.py) shows against float64 on the same inputs and at
least 16 eps32 - the factor 4 for the device's expf being a few ulps from NumPy's and for summation order.

  * decode boxes: |got - want| <= rtol * (|unclipped centre| + unclipped size) of that axis + FLT_MIN.  The error of a corner is made
    before the clip, relative to the centre and the size it is composed of; the clip is 1-Lipschitz, so a clipped coordinate needs no
    rule of its own;
  * decode probabilities: loss_judge.ratio / rtol_from elementwise, extra = 0;
  * suppression: keep lists and counts bit for bit; counts 0 outside [l_begin, l_end), rows outside it and entries past the count as
    pre-filled;
  * paste: EVERY pixel.  Outside the box window 0.  Inside, the reference's v64 >= 128, except where |v64 - 128| <= band: there either
    value passes.  band = 4 x the largest |v32 - v64| of the float32 oracle over the case's in-box pixels, at least 255 * 8 * 2^-24.

A helper of the tests, not a test and not part of the product."""
import numpy as np

from tests.loss_judge import EPS32, FLT_MIN, ratio, rtol_from  # noqa: F401

BAND_FLOOR = 255.0 * 8.0 * 2.0 ** -24


def box_scale(ref):
    """(R,4): |unclipped centre| + unclipped size of each coordinate's axis (y, x, y, x)."""
    s = np.abs(ref['centre']) + ref['size']
    return np.concatenate([s, s], 1)


def box_ratio(got, ref):
    """The smallest rtol with |got - want| <= rtol * box_scale + FLT_MIN everywhere."""
    got = np.asarray(got, np.float64)
    if got.shape != ref['bbox'].shape:
        raise ValueError('shapes differ: %s, %s' % (got.shape, ref['bbox'].shape))
    if not got.size:
        return 0.0
    over = np.maximum(np.abs(got - ref['bbox']) - FLT_MIN, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(over == 0, 0.0, over / box_scale(ref))
    return float(np.max(r))


def box_rtol(oracle_bbox, ref):
    return 4.0 * max(box_ratio(oracle_bbox, ref), 4.0 * EPS32)


def check_keep(keep_idx, keep_cnt, want, n_class, l_begin, l_end, fill=-1):
    """keep_idx (n_class, R) / keep_cnt (n_class,) of a device call against want = {l: indices}."""
    keep_idx, keep_cnt = np.asarray(keep_idx), np.asarray(keep_cnt)
    assert keep_cnt.shape == (n_class,) and keep_idx.shape[0] == n_class
    for l in range(n_class):
        if l_begin <= l < l_end:
            w = np.asarray(want[l])
            assert keep_cnt[l] == len(w), (l, int(keep_cnt[l]), len(w))
            np.testing.assert_array_equal(keep_idx[l, :len(w)], w, err_msg='class %d' % l)
            assert (keep_idx[l, len(w):] == fill).all(), l
        else:
            assert keep_cnt[l] == 0 and (keep_idx[l] == fill).all(), l


def paste_band(ref64, ref32):
    """4 x the float32 oracle's largest |v32 - v64| over the in-box pixels of the case, at least BAND_FLOOR; and that largest difference."""
    worst = 0.0
    for a, b in zip(ref64, ref32):
        if a['v'] is not None:
            worst = max(worst, float(np.abs(b['v'].astype(np.float64) - a['v']).max()))
    return max(4.0 * worst, BAND_FLOOR), worst


def paste_counts(ref64, band):
    """(in-box pixels, pixels of them with |v64 - 128| <= band) of a case."""
    n = k = 0
    for a in ref64:
        if a['v'] is not None:
            n += a['v'].size
            k += int((np.abs(a['v'] - 128.0) <= band).sum())
    return n, k


def check_paste(got, ref64, band):
    """got (D,H,W) of 0 / 1 (or bool) against the reference, pixel by pixel.  Returns the number of in-band pixels that were let pass."""
    got = np.asarray(got)
    assert got.shape[0] == len(ref64)
    assert ((got == 0) | (got == 1)).all()
    got = got.astype(bool)
    free = 0
    for i, a in enumerate(ref64):
        s, t, _, _, hh, ww = a['win']
        outside = got[i].copy()
        if a['v'] is not None:
            outside[s:s + hh, t:t + ww] = False
            want = a['v'] >= 128.0
            either = np.abs(a['v'] - 128.0) <= band
            bad = (got[i, s:s + hh, t:t + ww] != want) & ~either
            assert not bad.any(), ('detection %d: %d wrong pixels in its window, the first at %s, v64 = %r'
                                   % (i, int(bad.sum()), tuple(np.argwhere(bad)[0]), float(a['v'][tuple(np.argwhere(bad)[0])])))
            free += int(either.sum())
        assert not outside.any(), 'detection %d: %d pixels set outside its window, the first at %s' % (i, int(outside.sum()), tuple(np.argwhere(outside)[0]))
    return free
