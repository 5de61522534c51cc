"""Deformable convolution on the GPU (csrc/deform.hip, nn.core.DeformConv, the dcn_stages of the FPN and of MaskRCNN)
against tests/deform_reference.py evaluated in float64 from the same float32 inputs.

Bars.  The composed layer takes the convolution bars of tests/test_conv_paths_gpu.py, error = max|got - ref| / max|ref|: 1e-5 forward in
float32, 2e-5 backward data / filter in float32, 2e-6 for arithmetic 3 (the shipped arithmetic runs both backward passes with it and keeps a
backbone layer's forward pass in float32).  The three sampling kernels alone have no bar in the project: each case evaluates the reference in
float32 on the CPU, takes its error against float64 in the same norm and allows the kernel 4x that (a different but fixed summation order
over up to 64 channels and up to 315 list entries).  The values measured on an MI355X are listed beside KERNEL_CASES."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_reference as dr            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LD = 32                                     # the padded offset row
SHAPES = [(2, 5, 7, 32), (1, 1, 1, 32), (2, 6, 5, 64)]
SETS = ['a_zero', 'b_integer', 'c_fractional', 'd_one_cell', 'e_far', 'f_few_cells']
# The tiers of the input gradient's list handling, as csrc/deform.hip has them: up to RANK_MAX entries ordered by rank, up to LIST_MAX by the
# one-wave network in LDS, longer lists by a workgroup in chunks of LONG_CHUNK, LONG_WAVES chunks per round, LONG_GRID workgroups in all.
RANK_MAX, LIST_MAX, LONG_CHUNK, LONG_WAVES, LONG_GRID = 64, 256, 128, 8, 32
# a map large enough for lists beyond one round of chunks (9 H W = 5184 entries per image) and for more long lists than workgroups
LONG_SHAPE = (1, 24, 24, 32)
LONG_SETS = ['g_targets4', 'g_targets16']
PAD_FILL = 123.0                            # what the never-read channels of a test's offset row hold
FWD_TOL, BWD_TOL, ARITH3_TOL = 1e-5, 2e-5, 2e-6


def make_offsets(kind, shape, modulated, seed):
    """The offset row (N,H,W,LD) of one set, float32 on the CPU; channels past the 18 / 27 that are read hold PAD_FILL."""
    N, H, W, _ = shape
    g = torch.Generator().manual_seed(seed)
    off = torch.full((N, H, W, LD), PAD_FILL)
    d = torch.zeros((N, H, W, 9, 2))
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W, 1)
    ti = (torch.arange(9) // 3).float().view(1, 1, 1, 9)
    tj = (torch.arange(9) % 3).float().view(1, 1, 1, 9)
    if kind == 'b_integer':
        d = torch.randint(-2, 3, d.shape, generator=g).float()
        # positions exactly on -1 and on H / W: tap 0 of pixel (0, 0) and tap 8 of pixel (H-1, W-1) with zero offsets, and two forced ones
        d[:, 0, 0, 0] = 0
        d[:, H - 1, W - 1, 8] = 0
        d[:, H // 2, W // 2, 4, 0] = H - H // 2            # centre tap lands on row H exactly
        d[:, H // 2, W // 2, 3, 1] = -1 - (W // 2 - 1)     # tap (1, 0) lands on column -1 exactly
    elif kind == 'c_fractional':
        d = torch.randint(-2, 2, d.shape, generator=g).float() + (0.1 + 0.8 * torch.rand(d.shape, generator=g))
    elif kind == 'd_one_cell':                             # every tap of every pixel at the cell (H-1, W-1): one list of 9 H W entries
        d[..., 0] = (H - 1) - (ys - 1 + ti)
        d[..., 1] = (W - 1) - (xs - 1 + tj)
    elif kind == 'f_few_cells':
        # two taps in three aimed 0.3 / 0.6 of a cell inside one of two cells of their image, the third fractional as in (c): lists of some
        # 70 to 250 entries on eight destinations beside short ones in the same call
        d = torch.randint(-2, 2, d.shape, generator=g).float() + (0.1 + 0.8 * torch.rand(d.shape, generator=g))
        idx = torch.arange(H * W * 9).view(1, H, W, 9)
        aimed, second = (idx % 3 != 0).expand(N, H, W, 9), ((idx // 3) % 2 == 1).expand(N, H, W, 9)
        ty = torch.where(second, torch.tensor(float(max(H - 2, 0))), torch.tensor(0.0)) + 0.3
        tx = torch.where(second, torch.tensor(float(max(W - 2, 0))), torch.tensor(0.0)) + 0.6
        d[..., 0] = torch.where(aimed, ty - (ys - 1 + ti), d[..., 0])
        d[..., 1] = torch.where(aimed, tx - (xs - 1 + tj), d[..., 1])
    elif kind.startswith('g_targets'):
        # every tap of every pixel aimed 0.3 / 0.6 of a cell inside one of K cells on a grid, in turn: 4 K lists of 9 H W / K entries
        K = int(kind[len('g_targets'):])
        side = int(round(K ** 0.5))
        idx = torch.arange(H * W * 9).view(1, H, W, 9).expand(N, H, W, 9) % K
        ty = ((idx // side) * (H // side) + H // (2 * side)).float() + 0.3
        tx = ((idx % side) * (W // side) + W // (2 * side)).float() + 0.6
        d[..., 0] = ty - (ys - 1 + ti)
        d[..., 1] = tx - (xs - 1 + tj)
    elif kind == 'e_far':                                  # finite, up to 3 max(H, W), every position outside the map
        M = float(max(H, W))
        sign = torch.randint(0, 2, d.shape, generator=g).float() * 2 - 1
        d = sign * (2.5 + 0.5 * torch.rand(d.shape, generator=g)) * M
    off[..., :18] = d.reshape(N, H, W, 18)
    if modulated:
        off[..., 18:27] = 40.0 if kind == 'a_zero' else torch.randn((N, H, W, 9), generator=g)       # sigmoid(40) is 1.0f
    return off


def rel(got, ref):
    ref = ref.double()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


_CASE = {}


def kernel_case(shape, modulated, kind):
    """Inputs and float64 / float32 references of one case, computed once and shared by the tests that need them."""
    key = (shape, modulated, kind)
    if key not in _CASE:
        N, H, W, C = shape
        g = torch.Generator().manual_seed(1000 + sum(shape) + 7 * (SETS + LONG_SETS).index(kind) + int(modulated))
        c = {'x': torch.randn(shape, generator=g), 'g_cols': torch.randn((N, H, W, 9 * C), generator=g),
             'prior': torch.randn(shape, generator=g), 'relu_x': torch.randn(shape, generator=g).clamp_min(0),
             'off': make_offsets(kind, shape, modulated, 17 + sum(shape))}
        for name, dt in (('r64', torch.float64), ('r32', torch.float32)):
            cols, gx, goff = dr.cols_grads(c['x'], c['off'], c['g_cols'], modulated, dt)
            c[name] = {'cols': cols.reshape(N, H, W, 9 * C), 'gx': gx, 'goff': goff}
        _CASE[key] = c
    return _CASE[key]


def floor_and_bar(want32, want64):
    floor = rel(want32, want64)
    return floor, 4 * floor


# Measured on an MI355X: the reference's float32 error on the CPU -> the bar of 4x it (the kernel's error); of the four input-gradient
# variants the one closest to its bar.  A far (e) case compares exactly and has no bar; offset gradients are judged on the fractional set only.
#   shape            set           cols                           offset gradient                input gradient
#   (2,5,7,32)   v1  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                              7.47e-08 -> 2.99e-07 (7.47e-08)
#   (2,5,7,32)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                              1.06e-07 -> 4.24e-07 (1.21e-07)
#   (2,5,7,32)   v1  c_fractional  3.08e-07 -> 1.23e-06 (3.08e-07) 2.62e-07 -> 1.05e-06 (2.56e-07) 2.37e-07 -> 9.46e-07 (2.70e-07)
#   (2,5,7,32)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                              1.11e-07 -> 4.43e-07 (2.27e-07)
#   (2,5,7,32)   v1  f_few_cells   2.82e-07 -> 1.13e-06 (2.82e-07) -                              1.13e-07 -> 4.54e-07 (2.02e-07)
#   (2,5,7,32)   v2  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                              8.16e-08 -> 3.26e-07 (8.79e-08)
#   (2,5,7,32)   v2  b_integer     9.75e-08 -> 3.90e-07 (9.75e-08) -                              6.70e-08 -> 2.68e-07 (1.28e-07)
#   (2,5,7,32)   v2  c_fractional  2.59e-07 -> 1.04e-06 (2.59e-07) 3.36e-07 -> 1.35e-06 (3.36e-07) 2.28e-07 -> 9.11e-07 (2.25e-07)
#   (2,5,7,32)   v2  d_one_cell    9.28e-08 -> 3.71e-07 (9.28e-08) -                              1.19e-07 -> 4.75e-07 (2.43e-07)
#   (2,5,7,32)   v2  f_few_cells   4.13e-07 -> 1.65e-06 (4.13e-07) -                              1.19e-07 -> 4.78e-07 (3.04e-07)
#   (1,1,1,32)   v1  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                              3.38e-08 -> 1.35e-07 (3.38e-08)
#   (1,1,1,32)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                              0.00e+00 -> 0.00e+00 (0.00e+00)
#   (1,1,1,32)   v1  c_fractional  2.80e-08 -> 1.12e-07 (2.80e-08) 5.04e-08 -> 2.02e-07 (5.04e-08) 4.92e-08 -> 1.97e-07 (4.92e-08)
#   (1,1,1,32)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                              1.05e-07 -> 4.20e-07 (6.80e-08)
#   (1,1,1,32)   v1  f_few_cells   4.92e-08 -> 1.97e-07 (4.92e-08) -                              6.86e-08 -> 2.75e-07 (9.94e-08)
#   (1,1,1,32)   v2  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                              3.74e-08 -> 1.50e-07 (3.74e-08)
#   (1,1,1,32)   v2  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                              0.00e+00 -> 0.00e+00 (0.00e+00)
#   (1,1,1,32)   v2  c_fractional  4.16e-08 -> 1.66e-07 (4.16e-08) 1.96e-07 -> 7.85e-07 (4.36e-08) 2.28e-08 -> 9.14e-08 (3.21e-08)
#   (1,1,1,32)   v2  d_one_cell    8.11e-08 -> 3.24e-07 (8.11e-08) -                              8.34e-08 -> 3.34e-07 (1.10e-07)
#   (1,1,1,32)   v2  f_few_cells   5.99e-08 -> 2.39e-07 (5.68e-08) -                              2.73e-08 -> 1.09e-07 (7.70e-08)
#   (2,6,5,64)   v1  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                              1.03e-07 -> 4.12e-07 (1.03e-07)
#   (2,6,5,64)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                              8.07e-08 -> 3.23e-07 (1.15e-07)
#   (2,6,5,64)   v1  c_fractional  2.87e-07 -> 1.15e-06 (2.87e-07) 2.80e-07 -> 1.12e-06 (2.62e-07) 1.93e-07 -> 7.72e-07 (1.99e-07)
#   (2,6,5,64)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                              1.11e-07 -> 4.42e-07 (2.41e-07)
#   (2,6,5,64)   v1  f_few_cells   2.61e-07 -> 1.04e-06 (2.61e-07) -                              8.39e-08 -> 3.36e-07 (2.67e-07)
#   (2,6,5,64)   v2  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                              7.87e-08 -> 3.15e-07 (1.12e-07)
#   (2,6,5,64)   v2  b_integer     8.92e-08 -> 3.57e-07 (8.92e-08) -                              1.57e-07 -> 6.29e-07 (1.50e-07)
#   (2,6,5,64)   v2  c_fractional  2.97e-07 -> 1.19e-06 (2.97e-07) 2.56e-07 -> 1.03e-06 (2.62e-07) 2.17e-07 -> 8.66e-07 (2.79e-07)
#   (2,6,5,64)   v2  d_one_cell    7.80e-08 -> 3.12e-07 (7.80e-08) -                              1.26e-07 -> 5.05e-07 (3.16e-07)
#   (2,6,5,64)   v2  f_few_cells   2.54e-07 -> 1.02e-06 (2.54e-07) -                              1.24e-07 -> 4.97e-07 (2.16e-07)
#   (1,24,24,32) v1  g_targets4    7.81e-08 -> 3.12e-07 (7.81e-08) -                              2.22e-07 -> 8.88e-07 (2.24e-07)
#   (1,24,24,32) v1  g_targets16   9.48e-08 -> 3.79e-07 (9.48e-08) -                              1.34e-07 -> 5.36e-07 (3.31e-07)
#   (1,24,24,32) v2  g_targets4    1.15e-07 -> 4.60e-07 (1.15e-07) -                              2.14e-07 -> 8.58e-07 (2.53e-07)
#   (1,24,24,32) v2  g_targets16   1.34e-07 -> 5.37e-07 (1.34e-07) -                              1.59e-07 -> 6.37e-07 (2.33e-07)
KERNEL_CASES = [(s, m, k) for s in SHAPES for m in (False, True) for k in SETS]
LONG_CASES = [(LONG_SHAPE, m, k) for m in (False, True) for k in LONG_SETS]


def test_the_offset_sets_reach_every_tier_of_the_list_handling():
    """By the rule restated in tests/deform_reference.py, on the CPU: which list lengths each set gives the input gradient."""
    for shape in SHAPES:
        if shape[1] * shape[2] == 1:
            continue
        short = [int(dr.list_lengths(make_offsets(k, shape, False, 17 + sum(shape)), shape).max()) for k in ('a_zero', 'b_integer', 'c_fractional')]
        assert max(short) <= RANK_MAX, short                                                  # ordered by rank
        f = dr.list_lengths(make_offsets('f_few_cells', shape, False, 17 + sum(shape)), shape)
        assert RANK_MAX < int(f.max()) <= LIST_MAX and int(((f > RANK_MAX) & (f <= LIST_MAX)).sum()) >= 8, f.max()       # the network in LDS ...
        assert int(((f > 0) & (f <= RANK_MAX)).sum()) >= 8 and int((f > LIST_MAX).sum()) == 0                                # ... beside short lists
        d = dr.list_lengths(make_offsets('d_one_cell', shape, False, 17 + sum(shape)), shape)
        assert LIST_MAX < int(d.max()) <= LONG_CHUNK * LONG_WAVES                                 # the workgroup kernel, one round of chunks
    g4 = dr.list_lengths(make_offsets('g_targets4', LONG_SHAPE, False, 1), LONG_SHAPE)
    assert int(g4.max()) == 9 * 24 * 24 // 4 > LONG_CHUNK * LONG_WAVES and int((g4 > 0).sum()) == 16      # a second round of chunks
    g16 = dr.list_lengths(make_offsets('g_targets16', LONG_SHAPE, False, 1), LONG_SHAPE)
    assert int(g16.min() if (g16 > 0).all() else g16[g16 > 0].min()) > LIST_MAX and int((g16 > LIST_MAX).sum()) == 64 > LONG_GRID   # several long lists per workgroup


@pytest.mark.parametrize('shape,modulated,kind', KERNEL_CASES + LONG_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_sampling_kernels_alone(shape, modulated, kind):
    from chainer_maskrcnn._hip import ops
    c = kernel_case(shape, modulated, kind)
    N, H, W, C = shape
    used = 27 if modulated else 18
    x, off, g_cols = c['x'].to(DEV), c['off'].to(DEV), c['g_cols'].to(DEV)
    bad = []

    def judge(name, got, want64, want32):
        floor, bar = floor_and_bar(want32, want64)
        err = rel(got, want64)
        print('%-26s %s v%d %-12s err %.3e  cpu float32 %.3e  bar %.3e' % (name, shape, 2 if modulated else 1, kind, err, floor, bar))
        if not err <= bar:
            bad.append((name, err, bar))
    # the columns
    cols = ops.deform_cols_fwd(x, off, modulated)
    assert cols.shape == (N, H, W, 9 * C)
    if kind == 'e_far':
        assert not cols.any() and not c['r64']['cols'].any()
    else:
        judge('cols', cols, c['r64']['cols'], c['r32']['cols'])
    if kind == 'a_zero':        # the columns of zero offsets are the taps of the zero-padded input, exactly
        xp = F.pad(c['x'], (0, 0, 1, 1, 1, 1))
        want = torch.cat([xp[:, i:i + H, j:j + W] for i in range(3) for j in range(3)], 3)
        assert torch.equal(cols.cpu(), want)
    # the offset and mask gradient: the whole row, the padded channels exactly zero; its values where the sample is differentiable
    g_off = ops.deform_offset_bwd(g_cols, x, off, modulated)
    assert g_off.shape == (N, H, W, LD) and not g_off[..., used:].any()
    assert torch.equal(g_off, ops.deform_offset_bwd(g_cols, x, off, modulated))
    if kind == 'c_fractional':
        judge('offset gradient', g_off[..., :used], c['r64']['goff'][..., :used], c['r32']['goff'][..., :used])
        assert float(g_off[..., :used].abs().max()) > 0 and not c['r64']['goff'][..., used:].any()
    if kind == 'e_far':
        assert not g_off.any() and not c['r64']['goff'].any()
    # the input gradient: accumulate x relu_x, the mask on the total, the same bits twice
    prior, relu_x = c['prior'].to(DEV), c['relu_x'].to(DEV)
    keep = relu_x.cpu() > 0
    for acc in (False, True):
        for relu in (False, True):
            outs = [ops.deform_input_bwd(g_cols, off, modulated, shape, gx=prior.clone() if acc else None, relu_x=relu_x if relu else None)
                    for _ in range(2)]
            assert torch.equal(outs[0], outs[1])
            w64 = c['r64']['gx'] + (c['prior'].double() if acc else 0)
            w32 = c['r32']['gx'] + (c['prior'] if acc else 0)
            if relu:
                w64, w32 = w64 * keep, w32 * keep
                assert not outs[0].cpu()[~keep].any()
            if kind == 'e_far':
                want = (c['prior'] if acc else torch.zeros(shape)) * (keep if relu else 1)
                assert torch.equal(outs[0].cpu(), want) and not c['r64']['gx'].any()
            else:
                judge('input gradient acc%d relu%d' % (acc, relu), outs[0], w64, w32)
    if kind == 'd_one_cell':    # one destination per image holds every entry
        gx = ops.deform_input_bwd(g_cols, off, modulated, shape).cpu()
        assert gx[:, H - 1, W - 1].abs().min() > 0 and int((gx.abs().sum(3) > 0).sum()) == N
    assert not bad, bad


# ---- the composed layer ------------------------------------------------------------------------------------------------------------------
from chainer_maskrcnn.nn import core                                              # noqa: E402
from chainer_maskrcnn.nn.core import DeformConv, ParamStore                        # noqa: E402
from chainer_maskrcnn._hip import nn as hnn                                        # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import (DEFAULT_GEMM_ARITHMETIC, FPNMaskRCNNTrainChain, calc_mask_loss,      # noqa: E402
                                                             select_gemm_arithmetic)


class arithmetic(object):
    """'f32' or the shipped setting for the body, the library's defaults afterwards."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        select_gemm_arithmetic(self.name)

    def __exit__(self, *a):
        select_gemm_arithmetic('f32')


def backward_tol(name, pass_):
    """The bar of one pass under an arithmetic: the shipped one runs the backward passes of every layer with arithmetic 3 and keeps the
    forward pass of a backbone layer on the float32 MFMA."""
    if pass_ == 'fwd':
        return FWD_TOL
    return BWD_TOL if name == 'f32' else ARITH3_TOL


class PrescribedOffsets(object):
    """Stands where DeformConv's offset convolution stands and hands out a given offset row; keeps the gradient it is given."""

    def __init__(self, off):
        self.off, self.g_off = off, None

    def fwd(self, x, relu=False, tape=True):
        return self.off, ('prescribed',)

    def bwd(self, ctx, g_off, need_gx=True, gx_acc=None, accumulate_params=False):
        self.g_off = g_off
        if not need_gx:
            return None
        return gx_acc if gx_acc is not None else torch.zeros((g_off.shape[0], g_off.shape[1], g_off.shape[2], self.cin_p), device=g_off.device)


def _layer(C, Cout, modulated, seed=3):
    ps = ParamStore()
    dc = DeformConv(ps, 't/conv2', C, Cout, modulated=modulated, in_backbone=True)
    ps.materialise(torch.device(DEV), seed=seed)
    return ps, dc


@pytest.mark.parametrize('arith', ['f32', DEFAULT_GEMM_ARITHMETIC])
@pytest.mark.parametrize('shape,modulated,kind', KERNEL_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_composed_layer_with_prescribed_offsets(shape, modulated, kind, arith):
    c = kernel_case(shape, modulated, kind)
    N, H, W, C = shape
    used = 27 if modulated else 18
    ps, dc = _layer(C, C, modulated)
    stub = dc.offset = PrescribedOffsets(c['off'].to(DEV))
    stub.cin_p = C
    g = torch.Generator().manual_seed(5 + sum(shape))
    gy = torch.randn((N, H, W, C), generator=g)
    w = dc.W.cpu()
    y64, gx64, goff64, gw64 = dr.conv_grads(c['x'], c['off'], w, gy, modulated)
    x = c['x'].to(DEV)
    with arithmetic(arith):
        y, ctx = dc.fwd(x)
        gx = dc.bwd(ctx, gy.to(DEV))
        core.join_side_stream(torch.device(DEV))
        torch.cuda.synchronize()
        figures = [('forward', rel(y, y64), backward_tol(arith, 'fwd')), ('input gradient', rel(gx, gx64), backward_tol(arith, 'bwd')),
                   ('filter gradient', rel(dc.gW, gw64), backward_tol(arith, 'bwd'))]
        if kind == 'c_fractional':
            figures.append(('offset gradient', rel(stub.g_off[..., :used], goff64[..., :used]), backward_tol(arith, 'bwd')))
        if kind == 'a_zero':        # the plain 3x3 layer of the same filter
            plain = hnn.conv2d_fwd_raw(x, dc.W, None, 1, 1, False)
            figures.append(('against the plain layer', rel(y, plain.cpu()), FWD_TOL))
    if kind == 'e_far':
        assert not y.any() and not gx.any() and not dc.gW.any() and not stub.g_off.any()
        return
    assert not stub.g_off[..., used:].any()
    for name, err, tol in figures:
        print('%-24s %s v%d %-12s %-24s err %.3e bar %.1e' % (name, shape, 2 if modulated else 1, kind, arith, err, tol))
    assert all(err < tol for _, err, tol in figures), figures


def offset_conv64(x, w_off, b_off):
    return F.conv2d(x.double().permute(0, 3, 1, 2), w_off.double().permute(0, 3, 1, 2), b_off.double(), padding=1).permute(0, 2, 3, 1)


def layer_reference(x, off_used, w, w_off, b_off, gy, modulated):
    """float64 forward and gradients of the whole layer, the offset convolution included.  The sampling takes the offsets the layer itself
    used (``off_used``: the bars above are those of the sampling and its GEMM on given offsets; the offset convolution is held to its own
    bar by the caller) while the gradient flows through the float64 offset convolution."""
    x = x.detach().double().requires_grad_(True)
    w = w.detach().double().requires_grad_(True)
    w_off = w_off.detach().double().requires_grad_(True)
    b_off = b_off.detach().double().requires_grad_(True)
    o = offset_conv64(x, w_off, b_off)
    off = off_used.detach().double() + (o - o.detach())
    y = dr.deform_conv(x, off, w, modulated)
    gx, gw, gw_off, gb_off = torch.autograd.grad(y, (x, w, w_off, b_off), gy.double())
    return {'off': o.detach(), 'y': y.detach(), 'gx': gx, 'gw': gw, 'gw_off': gw_off, 'gb_off': gb_off}


def randomise_offset_conv(dc, seed):
    """Weights that give per-pixel offsets of about one cell: N(0, 1 / fan-in) on the logical rows, N(0, 0.25) biases; the pads stay zero."""
    g = torch.Generator().manual_seed(seed)
    w, b = dc.offset.W, dc.offset.b
    n, cin = dc.n_offset, dc.offset.cin
    w.zero_()
    b.zero_()
    w[:n, :, :, :cin] = (torch.randn((n, 3, 3, cin), generator=g) / (9 * cin) ** 0.5).to(w.device)
    b[:n] = (0.5 * torch.randn((n,), generator=g)).to(w.device)


@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_layer_with_its_offset_convolution(shape, modulated):
    """DeformConv with a trained-looking offset convolution, float32: forward, the four gradients, need_gx, gx_acc, mask_gx, tape=False, the
    padded rows of the offset filter's gradient, the same bits twice."""
    N, H, W, C = shape
    ps, dc = _layer(C, C, modulated)
    randomise_offset_conv(dc, 11)
    g = torch.Generator().manual_seed(23 + sum(shape))
    x = torch.randn(shape, generator=g).clamp_min(0)            # a ReLU output, as the layer's input is
    gy, prior = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xd, gyd = x.to(DEV), gy.to(DEV)
    n = dc.n_offset

    def run(**kw):
        ps.grads.zero_()
        y, ctx = dc.fwd(xd)
        gx = dc.bwd(ctx, gyd, **kw)
        core.join_side_stream(torch.device(DEV))
        torch.cuda.synchronize()
        return y, ctx, gx, {k: ps.g(k).clone() for k in ps.names()}
    y, ctx, gx, grads = run()
    off = ctx[1]
    assert off.shape == (N, H, W, LD) and not off[..., n:].any()
    ref = layer_reference(x, off.cpu(), dc.W.cpu(), dc.offset.W.cpu(), dc.offset.b.cpu(), gy, modulated)
    keep = x > 0
    figures = [('offsets', rel(off, ref['off']), FWD_TOL), ('forward', rel(y, ref['y']), FWD_TOL), ('input gradient', rel(gx, ref['gx']), BWD_TOL),
               ('filter gradient', rel(grads['t/conv2/W'], ref['gw']), BWD_TOL),
               ('offset filter gradient', rel(grads['t/conv2_offset/W'], ref['gw_off']), BWD_TOL),
               ('offset bias gradient', rel(grads['t/conv2_offset/b'], ref['gb_off']), BWD_TOL)]
    # the padded rows of the offset filter's gradient and of its bias gradient stay exactly zero
    assert not grads['t/conv2_offset/W'][n:].any() and not grads['t/conv2_offset/b'][n:].any()
    assert float(grads['t/conv2_offset/W'][:n].abs().max()) > 0
    # the same bits twice
    y2, _, gx2, grads2 = run()
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    # gx_acc with mask_gx: the prior value first, the mask on the total
    acc = prior.to(DEV)
    _, _, gx3, grads3 = run(gx_acc=acc, mask_gx=True)
    assert gx3 is acc and not gx3.cpu()[~keep].any() and all(torch.equal(grads[k], grads3[k]) for k in grads)
    figures.append(('accumulated, masked', rel(gx3, (ref['gx'] + prior.double()) * keep), BWD_TOL))
    # need_gx=False: parameter gradients only, the same bits
    _, _, gx4, grads4 = run(need_gx=False)
    assert gx4 is None and all(torch.equal(grads[k], grads4[k]) for k in grads)
    # tape=False: the same output, nothing kept
    y5, ctx5 = dc.fwd(xd, tape=False)
    assert ctx5 is None and torch.equal(y5, y)
    for name, err, tol in figures:
        print('%-24s %s v%d err %.3e bar %.1e' % (name, shape, 2 if modulated else 1, err, tol))
    assert all(err < tol for _, err, tol in figures), figures


# ---- inside the pyramid network ------------------------------------------------------------------------------------------------------------
from chainer_maskrcnn.model.extractor.feature_pyramid_network import FeaturePyramidNetwork       # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN                                             # noqa: E402
from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay                                 # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch                                          # noqa: E402

SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
ALL_STAGES = ('res3', 'res4', 'res5')


def _record(dc, rec):
    """Wraps the layer's two calls on the instance: what went in and what came out (clones: the block may overwrite either in place)."""
    fwd, bwd = dc.fwd, dc.bwd

    def fwd_(x, **kw):
        y, ctx = fwd(x, **kw)
        rec.update(x=x.clone(), y=y.clone(), off=ctx[1].clone())
        return y, ctx

    def bwd_(ctx, gy, **kw):
        rec.update(gy=gy.clone(), kw=kw)
        gx = bwd(ctx, gy, **kw)
        rec['gx'] = gx.clone()
        return gx
    dc.fwd, dc.bwd = fwd_, bwd_


@pytest.mark.parametrize('frozen', [False, True], ids=['batch_statistics', 'frozen_bn'])
@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
def test_deformable_blocks_inside_the_fpn(modulated, frozen):
    ext = FeaturePyramidNetwork(dcn_stages=ALL_STAGES, dcn_modulated=modulated, **SHRINK)
    ext.ps.materialise(torch.device(DEV), seed=5)
    if frozen:
        ext.set_freeze(bn=True, at=0)
    blocks = [ext.stages[si][0] for si in (1, 2, 3)]
    assert all(isinstance(b.conv2, DeformConv) and b.deform == ('v2' if modulated else 'v1') for b in blocks)
    assert not isinstance(ext.stages[0][0].conv2, DeformConv)
    recs = []
    for i, b in enumerate(blocks):
        randomise_offset_conv(b.conv2, 31 + i)
        recs.append({})
        _record(b.conv2, recs[-1])
    g = torch.Generator().manual_seed(77)
    img = torch.randn((2, 96, 128, 4), generator=g)
    img[..., 3] = 0
    outs = ext(img.to(DEV))
    ext.backward([torch.randn(o.shape, generator=g).to(DEV) for o in outs])
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()
    figures = []
    for b, r in zip(blocks, recs):
        dc = b.conv2
        assert r['kw'].get('mask_gx', False) == frozen and not dc.offset.W[dc.n_offset:].any()
        ref = layer_reference(r['x'].cpu(), r['off'].cpu(), dc.W.cpu(), dc.offset.W.cpu(), dc.offset.b.cpu(), r['gy'].cpu(), modulated)
        want_gx = ref['gx'] * (r['x'].cpu() > 0) if frozen else ref['gx']
        figures += [(dc.name, 'offsets', rel(r['off'], ref['off']), FWD_TOL), (dc.name, 'forward', rel(r['y'], ref['y']), FWD_TOL),
                    (dc.name, 'input gradient', rel(r['gx'], want_gx), BWD_TOL), (dc.name, 'filter gradient', rel(dc.gW, ref['gw']), BWD_TOL),
                    (dc.name, 'offset filter gradient', rel(dc.offset.gW, ref['gw_off']), BWD_TOL),
                    (dc.name, 'offset bias gradient', rel(ext.ps.g(dc.offset.name + '/b'), ref['gb_off']), BWD_TOL)]
        assert not dc.offset.gW[dc.n_offset:].any() and float(dc.offset.gW.abs().max()) > 0
    for f in figures:
        print('%-40s %-24s err %.3e bar %.1e' % f)
    assert all(f[2] < f[3] for f in figures), [f for f in figures if not f[2] < f[3]]


# ---- the whole model -------------------------------------------------------------------------------------------------------------------------
def _build(seed=7, **kw):
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=seed, _test_shrink=SHRINK, **kw)
    return m, FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss)


def _batch(N=2, H=128, W=160, G=3):
    b = make_batch(3, N, H, W, G=G)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [H, W])
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _step(chain, b):
    chain.sampler_keys = None
    chain.proposal_target_creator.set_seed(5)
    chain.anchor_target_creator.set_seed(9)
    chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0).backward()
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()


def _offset_names(m):
    return [n for n in m.ps.names() if '/conv2_offset/' in n]


@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
def test_training_step_and_predict(modulated):
    res = []
    for run in range(2):
        m, chain = _build(dcn_stages=ALL_STAGES, dcn_modulated=modulated, min_size=160, max_size=260)
        names = _offset_names(m)
        assert len(names) == 6 and not any(m.ps.p(n).any() for n in names)                 # zero-initialised
        b = _batch()
        _step(chain, b)
        obs = {k: float(v) for k, v in chain.observation.items()}
        assert all(np.isfinite(v) for v in obs.values()), obs
        assert torch.isfinite(m.ps.grads).all()
        for n in names:
            assert float(m.ps.g(n).abs().max()) > 0, n
        m.use_preset('evaluate')
        m.score_thresh = 0.0125                         # random weights: ~uniform class probabilities (1/81 = 0.0123)
        rs = np.random.RandomState(0)
        masks, labels, scores = m.predict([torch.from_numpy((rs.rand(3, 120, 150) * 255).astype(np.float32))])
        assert masks[0].shape[1:] == (120, 150) and torch.isfinite(scores[0]).all() and core.TRAIN is True
        res.append((m.ps.grads.clone(), obs, masks[0].clone(), labels[0].clone(), scores[0].clone()))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    assert all(torch.equal(res[0][i], res[1][i]) for i in (2, 3, 4))


def test_a_model_without_the_arguments_is_the_model_it_was():
    plain, _ = _build()
    off, _ = _build(dcn_stages=None, dcn_modulated=False)
    dcn, _ = _build(dcn_stages=ALL_STAGES)
    assert plain.ps.offsets == off.ps.offsets and torch.equal(plain.ps.params, off.ps.params)
    assert all(torch.equal(dcn.ps.p(n), plain.ps.p(n)) for n in plain.ps.names())          # every other parameter keeps its initial draw
    assert all(b.deform is None and not isinstance(b.conv2, DeformConv) for blocks in plain.extractor.stages for b in blocks)
    with pytest.raises(ValueError, match='dcn_stages'):
        MaskRCNN(n_fg_class=5, backbone='c4', head_arch='res5', device=DEV, _test_shrink=dict(width_div=4), dcn_stages=('res4',))


def test_graphed_step_replays_the_eager_step():
    from chainer_maskrcnn.optimizers import GraphedStep
    res = []
    for graphed in (False, True):
        m, chain = _build(dcn_stages=ALL_STAGES, dcn_modulated=True)
        b = _batch()
        chain.sampler_keys = None
        chain.proposal_target_creator.set_seed(5)
        chain.anchor_target_creator.set_seed(9)
        opt = MomentumSGD(lr=1e-2, momentum=0.9, high_priority_stream=False).setup(chain)
        opt.add_hook(WeightDecay(0.0005))
        batch = [b['imgs'], b['bboxes'], b['labels'], b['masks']]
        if graphed:
            g = GraphedStep(opt, chain, batch, 1.0, warmup=3)
            g(*batch)
        else:
            for _ in range(4):
                opt.update(chain, *batch, 1.0)
        torch.cuda.synchronize()
        res.append((m.ps.params.clone(), float(chain.observation['loss'])))
    assert res[0][1] == res[1][1] and torch.equal(res[0][0], res[1][0])
    assert any(m.ps.p(n).any() for n in _offset_names(m))                                   # four updates moved the offset convolutions
