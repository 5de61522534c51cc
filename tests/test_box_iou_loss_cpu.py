"""CPU tests of the IoU box regression losses (csrc/box_loss.hip, ops.box_iou_loss, FPNMaskRCNNTrainChain(box_loss=...); DESIGN.md section
3.20): the float64 restatement tests/box_iou_loss_reference.py against torch float64 autograd of the formulas written out here, the
clamp, the argument checks of the C ABI (no device), the chain's constructor and the flags of both training scripts."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import box_iou_loss_reference as ref  # noqa: E402
from chainer_maskrcnn import _hip  # noqa: E402

MEAN, STD, KINDS = ref.MEAN, ref.STD, ('giou', 'diou', 'ciou')
make_inputs, row_gaps = ref.make_inputs, ref.row_gaps


def torch_loss(x, t, rois, label, kind, mean, std, weight=1.0):
    """The formulas of the issue written out in torch (float64 tensors; x requires grad): corners, clamp(max=), alpha detached."""
    eps = 1e-7
    mean, std = torch.tensor(mean, dtype=x.dtype), torch.tensor(std, dtype=x.dtype)

    def corners(v, clamp):
        d = v * std + mean
        h, w = rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1]
        cy, cx = rois[:, 0] + 0.5 * h, rois[:, 1] + 0.5 * w
        dh, dw = (d[:, 2].clamp(max=ref.DSIZE_MAX), d[:, 3].clamp(max=ref.DSIZE_MAX)) if clamp else (d[:, 2], d[:, 3])
        ncy, ncx, nh, nw = d[:, 0] * h + cy, d[:, 1] * w + cx, torch.exp(dh) * h, torch.exp(dw) * w
        return ncy - 0.5 * nh, ncx - 0.5 * nw, ncy + 0.5 * nh, ncx + 0.5 * nw
    py1, px1, py2, px2 = corners(x, True)
    gy1, gx1, gy2, gx2 = corners(t, False)
    ih = (torch.minimum(py2, gy2) - torch.maximum(py1, gy1)).clamp(min=0)
    iw = (torch.minimum(px2, gx2) - torch.maximum(px1, gx1)).clamp(min=0)
    inter = ih * iw
    union = (py2 - py1) * (px2 - px1) + (gy2 - gy1) * (gx2 - gx1) - inter + eps
    iou = inter / union
    ch, cw = torch.maximum(py2, gy2) - torch.minimum(py1, gy1), torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    if kind == 'giou':
        L = 1 - iou + (ch * cw - union) / (ch * cw + eps)
    else:
        rho2 = ((py1 + py2) / 2 - (gy1 + gy2) / 2) ** 2 + ((px1 + px2) / 2 - (gx1 + gx2) / 2) ** 2
        L = 1 - iou + rho2 / (ch ** 2 + cw ** 2 + eps)
        if kind == 'ciou':
            v = 4 / math.pi ** 2 * (torch.atan((gx2 - gx1) / (gy2 - gy1 + eps)) - torch.atan((px2 - px1) / (py2 - py1 + eps))) ** 2
            alpha = (v / (1 - iou + v + eps)).detach()
            L = L + alpha * v
    pos = (label > 0).to(x.dtype)
    return weight * (L * pos).sum() / max(int((label >= 0).sum()), 1)


def _autograd(x, t, rois, label, kind, weight=1.0):
    xd = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    loss = torch_loss(xd, torch.from_numpy(t.astype(np.float64)), torch.from_numpy(rois.astype(np.float64)), torch.from_numpy(label), kind,
                      MEAN, STD, weight)
    loss.backward()
    return float(loss.detach()), xd.grad.numpy()


@pytest.mark.parametrize('kind', KINDS)
def test_reference_matches_torch_float64_autograd(kind):
    x, t, rois, label = make_inputs()
    assert row_gaps(x, t, rois).min() >= 1e-3            # no tie decides a subgradient
    assert (label > 0).sum() > 300 and (label == 0).any() and (label == -1).any()
    loss, count, g = ref.box_iou_loss(x, t, rois, label, kind, MEAN, STD, weight=2.5)
    want_loss, want_g = _autograd(x, t, rois, label, kind, weight=2.5)
    assert count == (label >= 0).sum()
    assert abs(loss - want_loss) <= 1e-10, (loss, want_loss)
    assert np.abs(g - want_g).max() <= 1e-10, np.abs(g - want_g).max()
    assert np.all(g[label <= 0] == 0) and np.abs(g[label > 0]).min(1).max() > 0
    # the inputs cover the geometry: disjoint and overlapping pairs, clamped and free sizes
    d = ref.decode(x, rois, MEAN, STD, clamp=True)[4][label > 0]
    assert (d[:, 2:] > ref.DSIZE_MAX).any() and (d[:, 2:] < ref.DSIZE_MAX).all(1).any()
    L = ref.rows(x, t, rois, 'giou', MEAN, STD)[0][label > 0]
    assert (L > 1.0).any() and (L < 0.3).any()


def test_reference_float32_run_is_close_to_float64():
    """The same code in float32 (the run that sets the GPU test's gradient bound) is the float64 result up to float32 rounding."""
    x, t, rois, label = make_inputs()
    for kind in KINDS:
        l64, _, g64 = ref.box_iou_loss(x, t, rois, label, kind, MEAN, STD)
        l32, _, g32 = ref.box_iou_loss(x, t, rois, label, kind, MEAN, STD, dtype=np.float32)
        assert g32.dtype == np.float32
        assert abs(l32 - l64) <= 1e-5 * l64
        assert np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max()


@pytest.mark.parametrize('kind', KINDS)
def test_roi_period_wraps_the_rois(kind):
    x, t, rois, label = make_inputs(M=40, seed=3)
    A = 8
    want = ref.box_iou_loss(x, t, rois[np.arange(40) % A], label, kind, MEAN, STD)
    got = ref.box_iou_loss(x, t, rois[:A], label, kind, MEAN, STD, roi_period=A)
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2])


@pytest.mark.parametrize('kind', KINDS)
def test_clamped_size_has_exactly_zero_gradient(kind):
    """dh above log(1000/16): column 2 of the gradient is exactly 0 in the reference and in autograd; at the bound itself it passes."""
    rois = np.array([[100., 100., 200., 180.]] * 3, np.float32)
    t = np.array([[0.3, -0.2, 0.5, 0.1]] * 3, np.float32)
    x = np.array([[0.1, 0.2, 80.0, 0.3], [0.1, 0.2, 0.4, 0.3], [0.1, 0.2, 0.0, 0.3]], np.float32)
    x[2, 2] = np.float32(ref.DSIZE_MAX) / np.float32(0.5)             # std 0.5: dh = DSIZE_MAX exactly
    label = np.ones(3, np.int32)
    std = (0.1, 0.1, 0.5, 0.2)
    _, _, g = ref.box_iou_loss(x, t, rois, label, kind, MEAN, std)
    xd = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    torch_loss(xd, torch.from_numpy(t.astype(np.float64)), torch.from_numpy(rois.astype(np.float64)), torch.from_numpy(label), kind, MEAN,
               std).backward()
    ga = xd.grad.numpy()
    assert float(np.float32(x[2, 2]) * np.float32(0.5)) == ref.DSIZE_MAX
    assert g[0, 2] == 0 and ga[0, 2] == 0
    assert g[1, 2] != 0 and g[2, 2] != 0 and ga[2, 2] != 0
    assert np.all(g[0, [1, 3]] != 0)                     # (the 6250 px tall box spans the target in y: GIoU's dy gradient is 0 too)
    np.testing.assert_allclose(g, ga, rtol=0, atol=1e-10)


@pytest.mark.parametrize('kind', KINDS)
def test_ties_split_the_derivative_like_autograd(kind):
    """Identical boxes (every min / max of the loss is a tie) and a prediction that shares two sides with its target: the reference splits
    the derivative of a tied min / max evenly, which is torch's rule, so it agrees with autograd there too - and identical boxes, the
    minimum of the loss, get a gradient of rounding size instead of a push from the kinks."""
    rois = np.array([[100., 200., 180., 300.]] * 2, np.float32)
    t = np.array([[0.5, -0.25, 1.0, 0.5]] * 2, np.float32)
    x = t.copy()
    x[1, 2] = 0.0                       # same centre and width, another height: both x sides tie
    label = np.array([1, 2], np.int32)
    assert row_gaps(x, t, rois).max() == 0
    _, _, g = ref.box_iou_loss(x, t, rois, label, kind, MEAN, STD)
    _, ga = _autograd(x, t, rois, label, kind)
    np.testing.assert_allclose(g, ga, rtol=0, atol=1e-10)
    assert np.abs(g[0]).max() <= 1e-9 and np.abs(g[1, 2]) > 1e-3


# ---- the C ABI: argument errors without a device ------------------------------------------------------------------------------------------
def _call(**kw):
    lib = _hip.lib()
    f4 = ctypes.c_float * 4
    one = ctypes.c_void_p(64)         # a non-null address that is never dereferenced: every case fails before a launch
    a = dict(x=one, ldx=4, t=one, rois=one, roi_period=5, label=one, M=5, kind=1, mean=f4(0, 0, 0, 0), std=f4(1, 1, 1, 1), weight=1.0,
             loss_out=one, gx=None, ldg=4, gfill=0, ws=one, ws_bytes=lib.mrcnn_loss_workspace_bytes())
    a.update(kw)
    return lib.mrcnn_box_iou_loss_f32(a['x'], a['ldx'], a['t'], a['rois'], a['roi_period'], a['label'], a['M'], a['kind'], a['mean'],
                                      a['std'], a['weight'], a['loss_out'], a['gx'], a['ldg'], a['gfill'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('bad', [dict(x=None), dict(t=None), dict(rois=None), dict(label=None), dict(ldx=3), dict(roi_period=0),
                                 dict(roi_period=-2), dict(kind=0), dict(kind=4), dict(loss_out=None), dict(ws=None), dict(mean=None),
                                 dict(std=None), dict(M=-1), dict(gx=ctypes.c_void_p(64), ldg=3),
                                 dict(gx=ctypes.c_void_p(64), ldg=4, gfill=8)],
                         ids=lambda b: ','.join('%s=%s' % (k, getattr(v, 'value', v)) for k, v in b.items()))
def test_bad_arguments_fail_before_any_launch(bad):
    lib = _hip.lib()
    assert _call(**bad) == -1
    msg = lib.mrcnn_last_error()
    assert b'box_iou_loss' in msg, msg


def test_short_workspace_is_refused():
    lib = _hip.lib()
    assert _call(ws_bytes=lib.mrcnn_loss_workspace_bytes() - 1) == -3
    assert b'box_iou_loss' in lib.mrcnn_last_error() and b'workspace' in lib.mrcnn_last_error()


def test_enum_values_and_abi_version():
    src = open(os.path.join(ROOT, 'include', 'mrcnn_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r'MRCNN_BOX_LOSS_([A-Z]+)\s*=\s*(\d+)', src)}
    assert got == {'GIOU': 1, 'DIOU': 2, 'CIOU': 3}
    assert (_hip.BOX_LOSS_GIOU, _hip.BOX_LOSS_DIOU, _hip.BOX_LOSS_CIOU) == (got['GIOU'], got['DIOU'], got['CIOU'])
    assert _hip.BOX_LOSS_KINDS == {'giou': 1, 'diou': 2, 'ciou': 3} == ref.KINDS
    assert 'mrcnn_box_iou_loss_f32' in _hip.SIGNATURES and len(_hip.SIGNATURES['mrcnn_box_iou_loss_f32'][1]) == 18
    assert _hip.ABI_VERSION == 10 and _hip.lib().mrcnn_abi_version() == 10
    assert re.search(r'#define MRCNN_ABI_VERSION 10\b', src)


def test_op_has_no_cpu_fallback():
    from chainer_maskrcnn._hip import ops
    z = torch.zeros(3, 4)
    with pytest.raises(_hip.MrcnnHipError):
        ops.box_iou_loss(z, 4, z, z, torch.ones(3, dtype=torch.int32), 3, 'giou', MEAN, STD)


# ---- the chain's constructor and the flags -------------------------------------------------------------------------------------------------
def _chain(**kw):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
    m = MaskRCNN(n_fg_class=80, device='cpu', seed=1, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=4))
    return FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, **kw)


def test_chain_constructor_checks_the_box_loss_arguments():
    c = _chain()
    assert (c.box_loss, c.rpn_box_loss, c.box_loss_weight, c.rpn_box_loss_weight) == ('smooth_l1', 'smooth_l1', 1.0, 1.0)
    c = _chain(box_loss='giou', rpn_box_loss='ciou', box_loss_weight=10, rpn_box_loss_weight=0.5)
    assert (c.box_loss, c.rpn_box_loss, c.box_loss_weight, c.rpn_box_loss_weight) == ('giou', 'ciou', 10.0, 0.5)
    assert _chain(box_loss='diou').rpn_box_loss == 'smooth_l1'
    for kw in (dict(box_loss='iou'), dict(rpn_box_loss='GIoU'), dict(box_loss=None), dict(rpn_box_loss=1)):
        with pytest.raises(ValueError, match='box_loss must be one of'):
            _chain(**kw)
    for w in (0, -1.0, float('nan'), float('inf'), '2', None, True):
        with pytest.raises(ValueError, match='box_loss_weight must be'):
            _chain(box_loss='giou', box_loss_weight=w)
        with pytest.raises(ValueError, match='rpn_box_loss_weight must be'):
            _chain(rpn_box_loss='giou', rpn_box_loss_weight=w)
    with pytest.raises(ValueError, match="box_loss='smooth_l1' takes 1.0 only"):
        _chain(box_loss_weight=2.0)
    with pytest.raises(ValueError, match="rpn_box_loss='smooth_l1' takes 1.0 only"):
        _chain(box_loss='giou', box_loss_weight=2.0, rpn_box_loss_weight=2.0)


def test_both_parsers_take_the_four_flags():
    import train
    for keypoints in (False, True):
        parser = train.build_parser(keypoints=keypoints)
        a = parser.parse_args([])
        assert (a.box_loss, a.rpn_box_loss, a.box_loss_weight, a.rpn_box_loss_weight) == ('smooth_l1', 'smooth_l1', 1.0, 1.0)
        a = parser.parse_args(['--box-loss', 'giou', '--rpn-box-loss', 'diou', '--box-loss-weight', '10', '--rpn-box-loss-weight', '2.5'])
        assert (a.box_loss, a.rpn_box_loss, a.box_loss_weight, a.rpn_box_loss_weight) == ('giou', 'diou', 10.0, 2.5)
        with pytest.raises(SystemExit):
            parser.parse_args(['--box-loss', 'iou'])
    a = train.build_parser(keypoints=True).parse_args(['--box_loss', 'ciou', '--rpn_box_loss_weight', '3'])     # both spellings
    assert a.box_loss == 'ciou' and a.rpn_box_loss_weight == 3.0
    with pytest.raises(ValueError, match="box_loss='smooth_l1' takes 1.0 only"):
        train.run(train.build_parser().parse_args(['--box-loss-weight', '2']))
