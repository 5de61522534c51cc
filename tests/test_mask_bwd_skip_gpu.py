"""GPU tests of the active-row mask of the mask branch's backward pass (csrc/conv.hip, csrc/planes_gemm.h,
csrc/targets.hip k_active_rows): the convolution backward entry points that take ``active`` must give the bits of the plain entry points
whenever gy is zero on the inactive images - they leave work out, they never change a sum.

Equality is ``torch.equal`` (-0 == +0): a skipped term is an exact zero of the dense pass, whose sign is the one thing that may differ.
Every masked call runs on a workspace poisoned with 0xFF bytes (NaN as float32 and as bf16): a row of V, W or M that the masked pipeline
left unwritten and still read would poison its result.

Shapes.  The issue's 48 maps of 14 x 14 x 256 are too few for the plane GEMMs on a 256-CU device: the data gradient's k_pgemm_pp wants
>= 256 tiles of 256 rows and a last round of CUs filled to 80 % (pg_big_ok), the filter gradient's k_pgemm_gpp >= 2048 tile rows
(pg_big_g_ok).  ``_plane_gemm_maps`` asks the dispatcher (mrcnn_conv2d_plan_query) for the smallest multiple of 48 maps at which both
passes take the plane GEMM - 192 on MI355X - and the cases assert that plan.  Blocks of 16 maps with n_pos = (16, 0, 5) repeated: a whole
256-row tile / 16-row K step active, a whole one inactive, a mixed one."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chainer_maskrcnn import _hip  # noqa: E402
from chainer_maskrcnn._hip import nn as hnn  # noqa: E402
from chainer_maskrcnn.nn import core  # noqa: E402

DEV = 'cuda:0'
BWD_DATA, BWD_FILTER = 1, 2


@contextlib.contextmanager
def bf16x6_backward():
    """The shipped arithmetic of the two backward passes (the plane GEMMs exist in it only); the library default afterwards."""
    lib = _hip.lib()
    try:
        _hip.check(lib.mrcnn_conv2d_set_split_operands(0, 3, 3))
        yield
    finally:
        _hip.check(lib.mrcnn_conv2d_set_split_operands(0, 0, 0))


def active_of(n_pos, rows_per_block):
    return (np.arange(len(n_pos) * rows_per_block) % rows_per_block < np.repeat(n_pos, rows_per_block)).astype(np.uint8)


def _plane_gemm_maps(H, C):
    for N in range(48, 48 * 9, 48):
        if all(hnn.conv_plan(p, (N, H, H, C), (C, 3, 3, C), 1, 1)['plane_gemm'] for p in (BWD_DATA, BWD_FILTER)):
            return N
    raise AssertionError('no batch up to 384 maps takes the plane GEMMs')


class Layer:
    """Operands of one layer; gy zero on the inactive images.  x is a ReLU output (relu_x)."""

    def __init__(self, N, H, Cin, Cout, K, n_pos, rows_per_block, seed=0):
        assert len(n_pos) * rows_per_block == N
        g = torch.Generator().manual_seed(seed + N + Cin)
        self.K, self.pad = K, K // 2
        self.x = torch.randn((N, H, H, Cin), generator=g).clamp_min(0).to(DEV)
        self.w = (torch.randn((Cout, K, K, Cin), generator=g) / (K * K * Cin) ** 0.5).to(DEV)
        act = active_of(np.asarray(n_pos), rows_per_block)
        self.gy = (torch.randn((N, H, H, Cout), generator=g) * torch.from_numpy(act).float().view(N, 1, 1, 1)).to(DEV)
        self.active = torch.from_numpy(act).to(DEV)
        self.base_x = torch.randn((N, H, H, Cin), generator=g).to(DEV)
        self.base_w = torch.randn((Cout, K, K, Cin), generator=g).to(DEV)
        self.base_b = torch.randn((Cout,), generator=g).to(DEV)
        # the device kernel's mask is the one the NumPy line gives
        n_pos_d = torch.tensor(list(n_pos), dtype=torch.int32, device=DEV)
        assert torch.equal(hnn.active_rows(n_pos_d, rows_per_block), self.active)

    def plan(self, pass_):
        return hnn.conv_plan(pass_, tuple(self.x.shape), tuple(self.w.shape), 1, self.pad)


def _poison():
    """0xFF into every cached workspace of this process (the calls below take theirs from that cache)."""
    for buf in hnn._ws_cache.values():
        buf.fill_(255)


def _data(L, active, relu_x=False, accumulate=False):
    out = L.base_x.clone() if accumulate else None
    if active is not None:
        _poison()
        if out is None:         # "nothing left unwritten": the call must overwrite every element of a fresh gx
            out_nan = torch.full_like(L.base_x, float('nan'))
            gx = _bwd_data_into(L, out_nan, relu_x, active)
            return gx
    return hnn.conv2d_bwd_data_raw(L.gy, L.w, tuple(L.x.shape), 1, L.pad, out=out, relu_x=L.x if relu_x else None, active=active)


def _bwd_data_into(L, gx, relu_x, active):
    """conv2d_bwd_data_raw without accumulation into a caller's (NaN-filled) tensor."""
    N, H, W, Cin = L.x.shape
    Cout, KH, KW, _ = L.w.shape
    nb = _hip.lib().mrcnn_conv2d_workspace_bytes(N, H, W, Cin, Cout, KH, KW, 1, L.pad)
    ws = hnn.workspace(nb, L.gy.device) if nb else None
    if ws is not None:
        ws.fill_(255)
    _hip.check(_hip.lib().mrcnn_conv2d_bwd_data_active_f32(
        _hip.ptr(L.gy), _hip.ptr(L.w), _hip.ptr(gx), _hip.ptr(L.x if relu_x else None), N, H, W, Cin, Cout, KH, KW, 1, L.pad, 0,
        _hip.ptr(active), active.numel(), _hip.ptr(ws), ws.numel() if ws is not None else 0, _hip.stream_ptr()))
    return gx


def _filter(L, active, accumulate=False):
    if accumulate:
        gw, gb = L.base_w.clone(), L.base_b.clone()
    else:
        gw, gb = torch.full_like(L.base_w, float('nan')), torch.full_like(L.base_b, float('nan'))
    if active is not None:
        _poison()
    hnn.conv2d_bwd_filter_raw(L.x, L.gy, tuple(L.w.shape), 1, L.pad, True, gw=gw, gb=gb, accumulate=accumulate, active=active)
    return gw, gb


def _check_layer(L, expect_plane_gemm):
    for p in (BWD_DATA, BWD_FILTER):
        assert bool(L.plan(p)['plane_gemm']) == expect_plane_gemm, (p, L.plan(p))
    for relu_x in (False, True):
        dense = _data(L, None, relu_x=relu_x)
        got = _data(L, L.active, relu_x=relu_x)
        assert torch.equal(got, dense), 'gx (relu_x=%s): %d elements differ' % (relu_x, int((got != dense).sum()))
        assert not bool(got[L.active == 0].any())
    dense = _data(L, None, accumulate=True)
    got = _data(L, L.active, accumulate=True)
    assert torch.equal(got, dense), 'gx accumulated'
    assert torch.equal(got[L.active == 0], L.base_x[L.active == 0])
    for accumulate in (False, True):
        gw0, gb0 = _filter(L, None, accumulate)
        gw1, gb1 = _filter(L, L.active, accumulate)
        assert torch.equal(gw1, gw0), 'gw (accumulate=%s): %d elements differ' % (accumulate, int((gw1 != gw0).sum()))
        assert torch.equal(gb1, gb0), 'gb (accumulate=%s)' % accumulate
    torch.cuda.synchronize()


@pytest.mark.parametrize('n_pos_kind', ['mixed', 'none', 'full'])
def test_winograd_plane_gemm_layer_equals_dense(n_pos_kind):
    """14 x 14 x 256 -> 256 in blocks of 16 maps: the transforms, k_pgemm_pp and k_pgemm_gpp with the mask against the same calls without."""
    with bf16x6_backward():
        N = _plane_gemm_maps(14, 256)
        nb = N // 16
        n_pos = {'mixed': [(16, 0, 5)[i % 3] for i in range(nb)], 'none': [0] * nb, 'full': [16] * nb}[n_pos_kind]
        L = Layer(N, 14, 256, 256, 3, n_pos, 16)
        _check_layer(L, True)
        if n_pos_kind == 'none':        # every output zero, the parameter gradients exactly zero, nothing left unwritten
            assert not bool(_data(L, L.active).any())
            gw, gb = _filter(L, L.active)
            assert not bool(gw.any()) and not bool(gb.any())


@pytest.mark.parametrize('H', [14, 20], ids=['direct', 'winograd_igemm'])
def test_small_layers_run_dense_and_equal(H):
    """64 -> 64 channels, 6 maps in blocks of 3, n_pos = (1, 0): 14 x 14 stays on the direct kernels, 20 x 20 takes F(4x4) with the
    k_conv_igemm GEMMs.  Neither has a plane GEMM: the mask travels with the call and the dense kernels run."""
    with bf16x6_backward():
        L = Layer(6, H, 64, 64, 3, (1, 0), 3)
        assert (L.plan(BWD_DATA)['path'] == 3) == (H == 20) and (L.plan(BWD_FILTER)['path'] == 3) == (H == 20)
        _check_layer(L, False)
        L0 = Layer(6, H, 64, 64, 3, (0, 0), 3)
        _check_layer(L0, False)
        gw, gb = _filter(L0, L0.active)
        assert not bool(gw.any()) and not bool(gb.any()) and not bool(_data(L0, L0.active).any())


def test_merged_deconvolution_pair_equals_dense():
    """The 1 x 1 layer 256 -> 4 * 96 of the merged deconvolution (k_conv_igemm in both passes), blocks of 16 maps."""
    with bf16x6_backward():
        L = Layer(48, 14, 256, 384, 1, (16, 0, 5), 16)
        _check_layer(L, False)


def test_wrong_mask_length_is_rejected():
    L = Layer(6, 14, 64, 64, 3, (1, 0), 3)
    with pytest.raises(_hip.MrcnnHipError):
        hnn.conv2d_bwd_data_raw(L.gy, L.w, tuple(L.x.shape), 1, 1, active=L.active[:5].contiguous())
    with pytest.raises(_hip.MrcnnHipError):
        hnn.conv2d_bwd_filter_raw(L.x, L.gy, tuple(L.w.shape), 1, 1, True, active=L.active[:5].contiguous())


@pytest.mark.parametrize('rows_per_block', [1, 3, 256])
def test_active_rows_kernel(rows_per_block):
    for n_pos in ([0, 0, 0], [rows_per_block] * 3, [0, rows_per_block, (rows_per_block + 1) // 2, min(1, rows_per_block)]):
        d = torch.tensor(n_pos, dtype=torch.int32, device=DEV)
        got = hnn.active_rows(d, rows_per_block).cpu().numpy()
        assert np.array_equal(got, active_of(np.asarray(n_pos), rows_per_block))


# ---- head level --------------------------------------------------------------------------------------------------------------------------
SCALES = [1 / 4., 1 / 8., 1 / 16., 1 / 32.]


def _head_run(head, xs, rois, levels, g_mask, active, on):
    keep = core.MASK_BWD_SKIP_INACTIVE
    core.MASK_BWD_SKIP_INACTIVE = on
    try:
        head.mask_branch(xs, rois, levels, SCALES)
        head.ps.grads.zero_()
        g_feats = [torch.ones_like(x) for x in xs]          # (the mask ROIAlign backward accumulates)
        _poison()
        g_pool = head.backward_mask_convs(g_mask, active=active)
        head.backward_mask_pool(g_pool, g_feats, active=active)
        core.join_side_stream(torch.device(DEV))
        torch.cuda.synchronize()
        return head.ps.grads.clone(), g_pool, g_feats
    finally:
        core.MASK_BWD_SKIP_INACTIVE = keep


def test_mask_head_backward_switch_on_equals_off():
    """2 images x 8 rows, 256 channels, n_pos = (3, 0): every parameter gradient, the pooled gradient and the pyramid gradients."""
    from chainer_maskrcnn.model.head.fpn_roi_mask_head import FPNRoIMaskHead
    with bf16x6_backward():
        head = FPNRoIMaskHead(5, roi_size_box=7, roi_size_mask=14, mask_initialW=0.01, in_channels=256, fc_channels=64)
        head.ps.materialise(torch.device(DEV), 3)
        g = torch.Generator().manual_seed(4)
        R = 16
        xs = [torch.randn((2, h, w, 256), generator=g).to(DEV) for h, w in ((16, 20), (8, 10), (4, 5), (2, 3))]
        y1, x1 = torch.rand(R, generator=g) * 30, torch.rand(R, generator=g) * 40
        hh, ww = 8 + torch.rand(R, generator=g) * 26, 8 + torch.rand(R, generator=g) * 32
        idx = (torch.arange(R) // 8).float()
        rois = torch.stack([idx, x1, y1, x1 + ww, y1 + hh], 1).to(DEV).contiguous()
        levels = torch.randint(0, 4, (R,), generator=g).to(torch.int32).to(DEV)
        active = hnn.active_rows(torch.tensor([3, 0], dtype=torch.int32, device=DEV), 8)
        S, Cm = head.mask_size, head.conv2.cout_p
        g_mask = torch.zeros((R, S, S, Cm))
        g_mask[..., :head.mask_out_channels] = torch.randn((R, S, S, head.mask_out_channels), generator=g)
        g_mask = (g_mask * active.cpu().float().view(R, 1, 1, 1)).to(DEV).contiguous()
        off = _head_run(head, xs, rois, levels, g_mask, active, False)
        on = _head_run(head, xs, rois, levels, g_mask, active, True)
        assert torch.equal(on[0], off[0]), 'parameter gradients: %d differ' % int((on[0] != off[0]).sum())
        assert torch.equal(on[1], off[1])
        assert all(torch.equal(a, b) for a, b in zip(on[2], off[2]))


# ---- step level --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width_div,arithmetic', [(2, None), (1, 'bf16x6_behind_backbone')], ids=['shrunk_f32', 'full_width_bf16x6'])
def test_step_switch_on_equals_off(width_div, arithmetic):
    """One mask_rows='all' step on the step tests' synthetic batch with the switch on and off: the losses and the flat gradient buffer.
    The shrunk model (128 channels, float32 MFMA) has no plane GEMM - the mask travels, the kernels run dense; at full width in the shipped
    arithmetic the mask convolutions (2 x 512 maps of 14 x 14 x 256) take k_pgemm_pp / k_pgemm_gpp and leave the inactive rows out."""
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import select_gemm_arithmetic
    from tests import step_harness
    keep = core.MASK_BWD_SKIP_INACTIVE
    res = {}
    try:
        m, chain = step_harness.build(dict(stages=(2, 1, 1, 1), width_div=width_div), 7, mask_rows='all',
                                      chain_kw={'gemm_arithmetic': arithmetic} if arithmetic else None)
        b = step_harness.batch()
        for on in (False, True):
            core.MASK_BWD_SKIP_INACTIVE = on
            m.ps.grads.zero_()
            _poison()
            step_harness.step(chain, b)
            assert (chain._mask_active is None)             # consumed by the backward pass
            res[on] = ([float(chain.observation[k]) for k in ('loss', 'mask_loss', 'roi_cls_loss', 'rpn_loc_loss')], m.ps.grads.clone())
            assert int(chain.targets['n_pos'].min()) < 512  # (some rows are inactive: the step has something to leave out)
    finally:
        core.MASK_BWD_SKIP_INACTIVE = keep
        select_gemm_arithmetic('f32')
    assert res[True][0] == res[False][0]
    assert bool(torch.isfinite(res[True][1]).all())
    assert torch.equal(res[True][1], res[False][1]), '%d gradient elements differ' % int((res[True][1] != res[False][1]).sum())
