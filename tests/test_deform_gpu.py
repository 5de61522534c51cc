"""Deformable convolution on the GPU (csrc/deform.hip, nn.core.DeformConv, the dcn_stages of the FPN and of MaskRCNN)
against tests/deform_reference.py evaluated in float64 from the same float32 inputs.

Cases.  tests/deform_cases.py holds the shapes, the offset sets and their generator, and restates the branches of csrc/deform.hip on the
channel count and on the pixel count; tests/test_deform_cases_cpu.py holds every case against the tier it is named for, without a device.
Beside the small shapes the three kernels run at the widths of res3 / res4 / res5 and at the widths next to every branch on C (128 | 132:
half a wave | a wave per (pixel, tap); 256 | 260 | 512: no lane | lane 0 | every lane with the second float4 accumulator of the input
gradient, 512 live threads in the long-list kernel; 516 and 1024: three and four trips of the channel loop, refused by the input gradient),
on maps of 1024 to 2400 pixels (one, two and three destinations per thread of the scan; long lists at both ends of it and in both images)
and on offset rows of stride 18 / 27, 20 / 28 and 40 beside the padded 32.

Bars.  The composed layer takes the convolution bars of tests/test_conv_paths_gpu.py, error = max|got - ref| / max|ref|: 1e-5 forward in
float32, 2e-5 backward data / filter in float32, 2e-6 for arithmetic 3 (the shipped arithmetic runs both backward passes with it and keeps a
backbone layer's forward pass in float32).  The three sampling kernels alone have no bar in the project: each case evaluates the reference in
float32 on the CPU, takes its error against float64 in the same norm and allows the kernel 4x that (a different but fixed summation order
over up to 1024 channels and up to 10800 list entries).  The values measured on an MI355X are listed beside KERNEL_CASES.  Where the
arithmetic does not depend on a size the comparison has NO bar: a column and an input-gradient channel depend on their own channel only and
are added in entry and chunk order whatever C is, so a wide call equals, bit for bit, the same call on 64-channel slices; an image's results
do not depend on the images beside it; nothing depends on the stride of the offset row."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_cases as cases             # noqa: E402
import deform_reference as dr            # noqa: E402
from deform_cases import (LD, LONG_SETS, LONG_SHAPE, OVER_WIDTHS, SCAN_CASES, SETS, SHAPES, STRIDE_SETS, STRIDE_SHAPE, STRIDES,      # noqa: E402
                          TWO_IMAGE_SHAPE, WIDE_LONG, WIDTH_MAP, WIDTH_SETS, WIDTHS, make_offsets, used_channels)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FWD_TOL, BWD_TOL, ARITH3_TOL = 1e-5, 2e-5, 2e-6
SENTINEL = -77.0                            # what a gx holds that a refused call must leave alone


def rel(got, ref):
    ref = ref.double()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


_CASE, _ONCE = {}, {}


def kernel_case(shape, modulated, kind):
    """Inputs and float64 / float32 references of one case, computed once and shared by the tests that need them; a case only one test
    needs (KEPT below says which are shared) is dropped when the next one is made."""
    key = (shape, modulated, kind)
    if key in _ONCE:
        return _ONCE[key]
    if key not in _CASE:
        N, H, W, C = shape
        g = torch.Generator().manual_seed(1000 + sum(shape) + 7 * (SETS + LONG_SETS).index(kind) + int(modulated))
        c = {'x': torch.randn(shape, generator=g), 'g_cols': torch.randn((N, H, W, 9 * C), generator=g),
             'prior': torch.randn(shape, generator=g), 'relu_x': torch.randn(shape, generator=g).clamp_min(0),
             'off': make_offsets(kind, shape, modulated, 17 + sum(shape))}
        for name, dt in (('r64', torch.float64), ('r32', torch.float32)):
            cols, gx, goff = dr.cols_grads(c['x'], c['off'], c['g_cols'], modulated, dt)
            c[name] = {'cols': cols.reshape(N, H, W, 9 * C), 'gx': gx, 'goff': goff}
        if key not in KEPT:
            _ONCE.clear()
            _ONCE[key] = c
            return c
        _CASE[key] = c
    return _CASE[key]


def floor_and_bar(want32, want64):
    floor = rel(want32, want64)
    return floor, 4 * floor


# Measured on an MI355X: the reference's float32 error on the CPU -> the bar of 4x it (the kernel's error); of the four input-gradient
# variants the one closest to its bar.  A far (e) case compares exactly and has no bar; offset gradients are judged on the fractional set only.
#   shape            set           cols                           offset gradient                input gradient
#   (2,5,7,32)    v1  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                               8.98e-08 -> 3.59e-07 (5.89e-08)
#   (2,5,7,32)    v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               9.27e-08 -> 3.71e-07 (6.18e-08)
#   (2,5,7,32)    v1  c_fractional  3.08e-07 -> 1.23e-06 (3.08e-07) 2.62e-07 -> 1.05e-06 (2.56e-07) 2.37e-07 -> 9.46e-07 (2.70e-07)
#   (2,5,7,32)    v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.26e-07 -> 5.04e-07 (7.03e-08)
#   (2,5,7,32)    v1  f_few_cells   2.82e-07 -> 1.13e-06 (2.82e-07) -                               1.12e-07 -> 4.49e-07 (6.28e-08)
#   (2,5,7,32)    v2  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                               9.73e-08 -> 3.89e-07 (6.01e-08)
#   (2,5,7,32)    v2  b_integer     9.75e-08 -> 3.90e-07 (9.75e-08) -                               6.88e-08 -> 2.75e-07 (6.47e-08)
#   (2,5,7,32)    v2  c_fractional  2.59e-07 -> 1.04e-06 (2.59e-07) 3.36e-07 -> 1.35e-06 (3.36e-07) 2.37e-07 -> 9.49e-07 (2.23e-07)
#   (2,5,7,32)    v2  d_one_cell    9.28e-08 -> 3.71e-07 (9.28e-08) -                               1.21e-07 -> 4.84e-07 (8.00e-08)
#   (2,5,7,32)    v2  f_few_cells   4.13e-07 -> 1.65e-06 (4.13e-07) -                               1.30e-07 -> 5.19e-07 (7.41e-08)
#   (1,1,1,32)    v1  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                               2.99e-08 -> 1.20e-07 (2.99e-08)
#   (1,1,1,32)    v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               0.00e+00 -> 0.00e+00 (0.00e+00)
#   (1,1,1,32)    v1  c_fractional  2.80e-08 -> 1.12e-07 (2.80e-08) 5.04e-08 -> 2.02e-07 (5.04e-08) 4.92e-08 -> 1.97e-07 (4.92e-08)
#   (1,1,1,32)    v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               9.41e-08 -> 3.76e-07 (4.47e-08)
#   (1,1,1,32)    v1  f_few_cells   4.92e-08 -> 1.97e-07 (4.92e-08) -                               6.33e-08 -> 2.53e-07 (7.93e-08)
#   (1,1,1,32)    v2  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                               3.74e-08 -> 1.50e-07 (3.74e-08)
#   (1,1,1,32)    v2  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               0.00e+00 -> 0.00e+00 (0.00e+00)
#   (1,1,1,32)    v2  c_fractional  4.16e-08 -> 1.66e-07 (4.16e-08) 1.96e-07 -> 7.85e-07 (4.36e-08) 2.28e-08 -> 9.14e-08 (3.21e-08)
#   (1,1,1,32)    v2  d_one_cell    8.11e-08 -> 3.24e-07 (8.11e-08) -                               7.80e-08 -> 3.12e-07 (7.62e-08)
#   (1,1,1,32)    v2  f_few_cells   5.99e-08 -> 2.39e-07 (5.68e-08) -                               2.73e-08 -> 1.09e-07 (4.35e-08)
#   (2,6,5,64)    v1  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.06e-07 -> 4.22e-07 (5.14e-08)
#   (2,6,5,64)    v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               8.07e-08 -> 3.23e-07 (8.07e-08)
#   (2,6,5,64)    v1  c_fractional  2.87e-07 -> 1.15e-06 (2.87e-07) 2.80e-07 -> 1.12e-06 (2.62e-07) 2.35e-07 -> 9.41e-07 (2.31e-07)
#   (2,6,5,64)    v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               8.39e-08 -> 3.36e-07 (4.92e-08)
#   (2,6,5,64)    v1  f_few_cells   2.61e-07 -> 1.04e-06 (2.61e-07) -                               8.92e-08 -> 3.57e-07 (7.46e-08)
#   (2,6,5,64)    v2  a_zero        0.00e+00 -> 0.00e+00 (0.00e+00) -                               7.87e-08 -> 3.15e-07 (5.08e-08)
#   (2,6,5,64)    v2  b_integer     8.92e-08 -> 3.57e-07 (8.92e-08) -                               1.57e-07 -> 6.29e-07 (9.22e-08)
#   (2,6,5,64)    v2  c_fractional  2.97e-07 -> 1.19e-06 (2.97e-07) 2.56e-07 -> 1.02e-06 (2.62e-07) 2.65e-07 -> 1.06e-06 (2.27e-07)
#   (2,6,5,64)    v2  d_one_cell    7.80e-08 -> 3.12e-07 (7.80e-08) -                               1.26e-07 -> 5.05e-07 (4.36e-08)
#   (2,6,5,64)    v2  f_few_cells   2.54e-07 -> 1.02e-06 (2.54e-07) -                               1.47e-07 -> 5.89e-07 (8.85e-08)
#   (1,24,24,32)  v1  g_targets4    7.81e-08 -> 3.12e-07 (7.81e-08) -                               2.31e-07 -> 9.24e-07 (9.92e-08)
#   (1,24,24,32)  v1  g_targets16   9.48e-08 -> 3.79e-07 (9.48e-08) -                               1.33e-07 -> 5.33e-07 (8.86e-08)
#   (1,24,24,32)  v2  g_targets4    1.15e-07 -> 4.60e-07 (1.15e-07) -                               2.38e-07 -> 9.54e-07 (1.42e-07)
#   (1,24,24,32)  v2  g_targets16   1.34e-07 -> 5.37e-07 (1.34e-07) -                               1.81e-07 -> 7.25e-07 (1.09e-07)
# The channel tiers (WIDTH_CASES); the input gradient refuses 516 and 1024 channels.
#   (2,5,7,128)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               7.77e-08 -> 3.11e-07 (6.38e-08)
#   (2,5,7,128)   v1  c_fractional  4.62e-07 -> 1.85e-06 (4.62e-07) 2.49e-07 -> 9.96e-07 (2.35e-07) 2.69e-07 -> 1.08e-06 (2.88e-07)
#   (2,5,7,128)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               9.51e-08 -> 3.80e-07 (5.55e-08)
#   (2,5,7,128)   v1  f_few_cells   3.76e-07 -> 1.50e-06 (3.76e-07) -                               9.76e-08 -> 3.91e-07 (6.78e-08)
#   (2,5,7,128)   v2  b_integer     9.17e-08 -> 3.67e-07 (9.17e-08) -                               8.99e-08 -> 3.60e-07 (6.53e-08)
#   (2,5,7,128)   v2  c_fractional  3.71e-07 -> 1.49e-06 (3.71e-07) 3.50e-07 -> 1.40e-06 (2.90e-07) 1.96e-07 -> 7.85e-07 (2.19e-07)
#   (2,5,7,128)   v2  d_one_cell    7.68e-08 -> 3.07e-07 (7.68e-08) -                               1.35e-07 -> 5.38e-07 (9.03e-08)
#   (2,5,7,128)   v2  f_few_cells   3.06e-07 -> 1.22e-06 (3.06e-07) -                               1.46e-07 -> 5.83e-07 (9.36e-08)
#   (2,5,7,132)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.20e-07 -> 4.80e-07 (5.51e-08)
#   (2,5,7,132)   v1  c_fractional  3.76e-07 -> 1.51e-06 (3.76e-07) 2.29e-07 -> 9.16e-07 (1.96e-07) 1.86e-07 -> 7.45e-07 (1.86e-07)
#   (2,5,7,132)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               9.95e-08 -> 3.98e-07 (5.42e-08)
#   (2,5,7,132)   v1  f_few_cells   2.86e-07 -> 1.15e-06 (2.86e-07) -                               1.43e-07 -> 5.70e-07 (8.85e-08)
#   (2,5,7,132)   v2  b_integer     8.85e-08 -> 3.54e-07 (8.85e-08) -                               1.08e-07 -> 4.31e-07 (9.16e-08)
#   (2,5,7,132)   v2  c_fractional  3.49e-07 -> 1.40e-06 (3.49e-07) 2.50e-07 -> 1.00e-06 (2.78e-07) 2.15e-07 -> 8.60e-07 (1.89e-07)
#   (2,5,7,132)   v2  d_one_cell    1.00e-07 -> 4.00e-07 (1.00e-07) -                               1.15e-07 -> 4.60e-07 (1.10e-07)
#   (2,5,7,132)   v2  f_few_cells   3.61e-07 -> 1.44e-06 (3.61e-07) -                               1.14e-07 -> 4.54e-07 (9.75e-08)
#   (2,5,7,256)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.12e-07 -> 4.49e-07 (6.82e-08)
#   (2,5,7,256)   v1  c_fractional  3.81e-07 -> 1.52e-06 (3.81e-07) 4.06e-07 -> 1.62e-06 (2.68e-07) 2.22e-07 -> 8.90e-07 (2.22e-07)
#   (2,5,7,256)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.12e-07 -> 4.47e-07 (8.18e-08)
#   (2,5,7,256)   v1  f_few_cells   2.97e-07 -> 1.19e-06 (2.97e-07) -                               1.18e-07 -> 4.72e-07 (7.00e-08)
#   (2,5,7,256)   v2  b_integer     7.60e-08 -> 3.04e-07 (7.94e-08) -                               8.77e-08 -> 3.51e-07 (8.11e-08)
#   (2,5,7,256)   v2  c_fractional  4.74e-07 -> 1.90e-06 (4.74e-07) 2.12e-07 -> 8.49e-07 (1.87e-07) 1.95e-07 -> 7.80e-07 (1.95e-07)
#   (2,5,7,256)   v2  d_one_cell    1.04e-07 -> 4.14e-07 (1.04e-07) -                               1.75e-07 -> 7.00e-07 (7.91e-08)
#   (2,5,7,256)   v2  f_few_cells   4.46e-07 -> 1.79e-06 (4.46e-07) -                               1.44e-07 -> 5.74e-07 (9.49e-08)
#   (2,5,7,260)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               9.64e-08 -> 3.86e-07 (6.92e-08)
#   (2,5,7,260)   v1  c_fractional  3.55e-07 -> 1.42e-06 (3.55e-07) 2.53e-07 -> 1.01e-06 (2.81e-07) 2.57e-07 -> 1.03e-06 (2.55e-07)
#   (2,5,7,260)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.22e-07 -> 4.87e-07 (8.17e-08)
#   (2,5,7,260)   v1  f_few_cells   3.94e-07 -> 1.57e-06 (3.94e-07) -                               9.49e-08 -> 3.80e-07 (6.21e-08)
#   (2,5,7,260)   v2  b_integer     8.05e-08 -> 3.22e-07 (8.05e-08) -                               1.02e-07 -> 4.08e-07 (9.90e-08)
#   (2,5,7,260)   v2  c_fractional  4.36e-07 -> 1.75e-06 (4.36e-07) 2.54e-07 -> 1.02e-06 (2.54e-07) 2.30e-07 -> 9.20e-07 (2.02e-07)
#   (2,5,7,260)   v2  d_one_cell    9.15e-08 -> 3.66e-07 (9.15e-08) -                               1.15e-07 -> 4.62e-07 (7.60e-08)
#   (2,5,7,260)   v2  f_few_cells   4.48e-07 -> 1.79e-06 (4.48e-07) -                               1.16e-07 -> 4.63e-07 (9.24e-08)
#   (2,5,7,512)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.18e-07 -> 4.72e-07 (5.46e-08)
#   (2,5,7,512)   v1  c_fractional  4.21e-07 -> 1.69e-06 (4.21e-07) 3.16e-07 -> 1.26e-06 (2.32e-07) 2.96e-07 -> 1.19e-06 (2.96e-07)
#   (2,5,7,512)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               1.67e-07 -> 6.67e-07 (6.94e-08)
#   (2,5,7,512)   v1  f_few_cells   3.50e-07 -> 1.40e-06 (3.50e-07) -                               1.58e-07 -> 6.33e-07 (1.11e-07)
#   (2,5,7,512)   v2  b_integer     9.63e-08 -> 3.85e-07 (9.22e-08) -                               1.09e-07 -> 4.36e-07 (7.74e-08)
#   (2,5,7,512)   v2  c_fractional  3.23e-07 -> 1.29e-06 (3.23e-07) 3.74e-07 -> 1.49e-06 (3.74e-07) 2.07e-07 -> 8.29e-07 (2.20e-07)
#   (2,5,7,512)   v2  d_one_cell    8.71e-08 -> 3.49e-07 (8.71e-08) -                               1.23e-07 -> 4.94e-07 (8.80e-08)
#   (2,5,7,512)   v2  f_few_cells   3.89e-07 -> 1.56e-06 (3.89e-07) -                               1.70e-07 -> 6.81e-07 (1.29e-07)
#   (2,5,7,516)   v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               refused
#   (2,5,7,516)   v1  c_fractional  3.71e-07 -> 1.48e-06 (3.71e-07) 2.69e-07 -> 1.08e-06 (2.97e-07) refused
#   (2,5,7,516)   v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               refused
#   (2,5,7,516)   v1  f_few_cells   3.53e-07 -> 1.41e-06 (3.53e-07) -                               refused
#   (2,5,7,516)   v2  b_integer     9.04e-08 -> 3.62e-07 (9.04e-08) -                               refused
#   (2,5,7,516)   v2  c_fractional  4.52e-07 -> 1.81e-06 (4.52e-07) 3.26e-07 -> 1.31e-06 (2.63e-07) refused
#   (2,5,7,516)   v2  d_one_cell    9.16e-08 -> 3.66e-07 (9.16e-08) -                               refused
#   (2,5,7,516)   v2  f_few_cells   4.07e-07 -> 1.63e-06 (4.07e-07) -                               refused
#   (2,5,7,1024)  v1  b_integer     0.00e+00 -> 0.00e+00 (0.00e+00) -                               refused
#   (2,5,7,1024)  v1  c_fractional  4.89e-07 -> 1.96e-06 (4.89e-07) 2.36e-07 -> 9.42e-07 (2.67e-07) refused
#   (2,5,7,1024)  v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               refused
#   (2,5,7,1024)  v1  f_few_cells   3.71e-07 -> 1.48e-06 (3.71e-07) -                               refused
#   (2,5,7,1024)  v2  b_integer     8.96e-08 -> 3.58e-07 (8.96e-08) -                               refused
#   (2,5,7,1024)  v2  c_fractional  3.10e-07 -> 1.24e-06 (3.10e-07) 2.80e-07 -> 1.12e-06 (2.58e-07) refused
#   (2,5,7,1024)  v2  d_one_cell    9.98e-08 -> 3.99e-07 (9.98e-08) -                               refused
#   (2,5,7,1024)  v2  f_few_cells   3.66e-07 -> 1.46e-06 (3.66e-07) -                               refused
#   (1,24,24,512) v1  g_targets4    8.17e-08 -> 3.27e-07 (8.17e-08) -                               2.84e-07 -> 1.14e-06 (1.54e-07)
#   (1,24,24,512) v2  g_targets4    1.38e-07 -> 5.53e-07 (1.38e-07) -                               2.40e-07 -> 9.59e-07 (1.40e-07)
# The scan beyond one destination per thread (SCAN_KERNEL_CASES); positions up to 41 have a coarser float32 grid than those of a 5 x 7 map.
#   (1,32,32,32)  v1  c_fractional  1.48e-06 -> 5.90e-06 (1.48e-06) 1.50e-06 -> 5.99e-06 (1.50e-06) 1.26e-06 -> 5.05e-06 (1.27e-06)
#   (1,32,32,32)  v2  c_fractional  1.59e-06 -> 6.36e-06 (1.59e-06) 1.42e-06 -> 5.70e-06 (1.41e-06) 1.48e-06 -> 5.93e-06 (1.48e-06)
#   (1,25,41,32)  v1  c_fractional  2.73e-06 -> 1.09e-05 (2.73e-06) 2.17e-06 -> 8.67e-06 (2.10e-06) 1.91e-06 -> 7.63e-06 (1.92e-06)
#   (1,25,41,32)  v2  c_fractional  2.79e-06 -> 1.12e-05 (2.79e-06) 2.54e-06 -> 1.02e-05 (2.50e-06) 1.62e-06 -> 6.48e-06 (1.62e-06)
#   (1,33,32,32)  v1  c_fractional  1.62e-06 -> 6.47e-06 (1.62e-06) 1.32e-06 -> 5.27e-06 (1.30e-06) 1.16e-06 -> 4.65e-06 (1.15e-06)
#   (1,33,32,32)  v1  g_targets16   8.50e-08 -> 3.40e-07 (8.50e-08) -                               2.86e-07 -> 1.14e-06 (1.13e-07)
#   (1,33,32,32)  v2  c_fractional  1.29e-06 -> 5.17e-06 (1.29e-06) 1.20e-06 -> 4.80e-06 (1.22e-06) 1.35e-06 -> 5.41e-06 (1.38e-06)
#   (1,33,32,32)  v2  g_targets16   1.49e-07 -> 5.94e-07 (1.49e-07) -                               2.44e-07 -> 9.78e-07 (1.06e-07)
#   (2,40,30,32)  v1  c_fractional  2.64e-06 -> 1.06e-05 (2.64e-06) 2.01e-06 -> 8.05e-06 (1.96e-06) 1.46e-06 -> 5.86e-06 (1.49e-06)
#   (2,40,30,32)  v1  d_one_cell    0.00e+00 -> 0.00e+00 (0.00e+00) -                               5.16e-07 -> 2.06e-06 (2.11e-07)
#   (2,40,30,32)  v1  f_few_cells   2.80e-06 -> 1.12e-05 (2.80e-06) -                               5.36e-07 -> 2.15e-06 (2.16e-07)
#   (2,40,30,32)  v2  c_fractional  2.48e-06 -> 9.90e-06 (2.48e-06) 1.70e-06 -> 6.81e-06 (1.68e-06) 1.82e-06 -> 7.29e-06 (1.86e-06)
#   (2,40,30,32)  v2  d_one_cell    1.33e-07 -> 5.33e-07 (1.33e-07) -                               5.07e-07 -> 2.03e-06 (3.44e-07)
#   (2,40,30,32)  v2  f_few_cells   2.89e-06 -> 1.16e-05 (2.89e-06) -                               5.56e-07 -> 2.22e-06 (2.58e-07)
KERNEL_CASES = [(s, m, k) for s in SHAPES for m in (False, True) for k in SETS]
LONG_CASES = [(LONG_SHAPE, m, k) for m in (False, True) for k in LONG_SETS]
# the channel tiers, the scan beyond one destination per thread (tests/deform_cases.py)
WIDTH_CASES = ([(WIDTH_MAP + (C,), m, k) for C in WIDTHS + OVER_WIDTHS for m in (False, True) for k in WIDTH_SETS]
               + [(WIDE_LONG[0], m, WIDE_LONG[1]) for m in (False, True)])
SCAN_KERNEL_CASES = [(s, m, k) for s, kinds in SCAN_CASES for m in (False, True) for k in kinds]
COMPOSED_WIDE_CASES = [(WIDTH_MAP + (C,), m, k) for C in (128, 256, 512) for m in (False, True) for k in ('a_zero', 'c_fractional')]
STRIDE_CASES = [(STRIDE_SHAPE, m, k) for m in (False, True) for k in STRIDE_SETS]
KEPT = set(KERNEL_CASES + COMPOSED_WIDE_CASES + STRIDE_CASES)           # the cases more than one test asks for
VARIANTS = [(acc, relu) for acc in (False, True) for relu in (False, True)]


def run_kernels(x, off, g_cols, prior, relu_x, modulated, input_gradient=True):
    """The three kernels on device tensors: the columns, the offset gradient, the input gradient in the four accumulate x relu_x variants;
    every backward call twice for the same bits."""
    from chainer_maskrcnn._hip import ops
    shape = tuple(x.shape)
    out = {'cols': ops.deform_cols_fwd(x, off, modulated), 'g_off': ops.deform_offset_bwd(g_cols, x, off, modulated)}
    assert torch.equal(out['g_off'], ops.deform_offset_bwd(g_cols, x, off, modulated))
    if input_gradient:
        for acc, relu in VARIANTS:
            outs = [ops.deform_input_bwd(g_cols, off, modulated, shape, gx=prior.clone() if acc else None, relu_x=relu_x if relu else None)
                    for _ in range(2)]
            assert torch.equal(outs[0], outs[1])
            out[(acc, relu)] = outs[0]
    return out


def device_inputs(c, channels=None, image=None):
    """x, off, g_cols, prior, relu_x of a case on the device; `channels`: a slice of the channels, `image`: one image of the batch."""
    N, H, W, C = c['x'].shape
    ch = channels if channels is not None else slice(0, C)
    im = slice(image, image + 1) if image is not None else slice(0, N)
    n, w = im.stop - im.start, ch.stop - ch.start
    g_cols = c['g_cols'].view(N, H, W, 9, C)[im, :, :, :, ch].reshape(n, H, W, 9 * w)
    return [t.contiguous().to(DEV) for t in (c['x'][im, :, :, ch], c['off'][im], g_cols, c['prior'][im, :, :, ch], c['relu_x'][im, :, :, ch])]


@pytest.mark.parametrize('shape,modulated,kind', KERNEL_CASES + LONG_CASES + WIDTH_CASES + SCAN_KERNEL_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_sampling_kernels_alone(shape, modulated, kind):
    from chainer_maskrcnn._hip import MrcnnHipError, ops
    c = kernel_case(shape, modulated, kind)
    N, H, W, C = shape
    used = used_channels(modulated)
    refused = C > cases.C_MAX               # the input gradient takes at most C_MAX channels; the other two kernels loop
    x, off, g_cols, prior, relu_x = device_inputs(c)
    bad = []

    def judge(name, got, want64, want32):
        floor, bar = floor_and_bar(want32, want64)
        err = rel(got, want64)
        print('%-26s %s v%d %-12s err %.3e  cpu float32 %.3e  bar %.3e' % (name, shape, 2 if modulated else 1, kind, err, floor, bar))
        if not err <= bar:
            bad.append((name, err, bar))
    got = run_kernels(x, off, g_cols, prior, relu_x, modulated, input_gradient=not refused)
    # the columns
    cols = got['cols']
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
    g_off = got['g_off']
    assert g_off.shape == (N, H, W, LD) and not g_off[..., used:].any()
    if kind == 'c_fractional':
        judge('offset gradient', g_off[..., :used], c['r64']['goff'][..., :used], c['r32']['goff'][..., :used])
        assert float(g_off[..., :used].abs().max()) > 0 and not c['r64']['goff'][..., used:].any()
    if kind == 'e_far':
        assert not g_off.any() and not c['r64']['goff'].any()
    # the input gradient: accumulate x relu_x, the mask on the total, the same bits twice
    keep = c['relu_x'] > 0
    for acc, relu in ([] if refused else VARIANTS):
        out = got[(acc, relu)]
        w64 = c['r64']['gx'] + (c['prior'].double() if acc else 0)
        w32 = c['r32']['gx'] + (c['prior'] if acc else 0)
        if relu:
            w64, w32 = w64 * keep, w32 * keep
            assert not out.cpu()[~keep].any()
        if kind == 'e_far':
            want = (c['prior'] if acc else torch.zeros(shape)) * (keep if relu else 1)
            assert torch.equal(out.cpu(), want) and not c['r64']['gx'].any()
        else:
            judge('input gradient acc%d relu%d' % (acc, relu), out, w64, w32)
    if refused:                 # before any launch: every variant raises, and the gx a call was given stays full of its sentinel
        for acc, relu in VARIANTS:
            gx = torch.full(shape, SENTINEL, device=DEV) if acc else None
            with pytest.raises(MrcnnHipError, match='at most %d' % cases.C_MAX):
                ops.deform_input_bwd(g_cols, off, modulated, shape, gx=gx, relu_x=relu_x if relu else None)
            torch.cuda.synchronize()
            assert gx is None or bool((gx == SENTINEL).all())
    elif kind == 'd_one_cell':  # one destination per image holds every entry
        gx = got[(False, False)].cpu()
        assert gx[:, H - 1, W - 1].abs().min() > 0 and int((gx.abs().sum(3) > 0).sum()) == N
    # a wide call against the same call on 64-channel slices, bit for bit: a column and an input-gradient channel depend on their own
    # channel only and the additions run in entry and chunk order whatever C is (the offset gradient sums over the channels: no such rule)
    if C > cases.SLICE:
        cols5 = cols.view(N, H, W, 9, C)
        for s in cases.slice_starts(C):
            ch = slice(s, s + cases.SLICE)
            part = run_kernels(*device_inputs(c, channels=ch), modulated, input_gradient=not refused)
            assert torch.equal(cols5[..., ch], part['cols'].view(N, H, W, 9, cases.SLICE)), ('cols', s)
            for v in ([] if refused else VARIANTS):
                assert torch.equal(got[v][..., ch], part[v]), ('input gradient', v, s)
    # a batch against its images one at a time, bit for bit: the order of a destination's entries does not change with the image offset
    if shape == TWO_IMAGE_SHAPE:
        for n in range(N):
            part = run_kernels(*device_inputs(c, image=n), modulated)
            assert torch.equal(cols[n:n + 1], part['cols']) and torch.equal(g_off[n:n + 1], part['g_off']), n
            for v in VARIANTS:
                assert torch.equal(got[v][n:n + 1], part[v]), ('input gradient', v, n)
    assert not bad, bad


@pytest.mark.parametrize('ld_index', [0, 1, 2], ids=['unpadded', 'next4', 'wide'])
@pytest.mark.parametrize('shape,modulated,kind', STRIDE_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_offset_row_strides(shape, modulated, kind, ld_index):
    """The kernels take the stride of the offset row: 18 / 27 (no padded channel, rows not 16-byte aligned), 20 / 28 and 40 give the bits of
    the padded row of 32 on the same values; the channels behind the used ones are exactly zero; g_off has the given stride."""
    c = kernel_case(shape, modulated, kind)
    N, H, W, C = shape
    used, ld = used_channels(modulated), STRIDES[modulated][ld_index]
    x, off, g_cols, prior, relu_x = device_inputs(c)
    want = run_kernels(x, off, g_cols, prior, relu_x, modulated)
    row = make_offsets(kind, shape, modulated, cases.offset_seed(shape), ld=ld)
    assert row.shape == (N, H, W, ld) and ld >= used and torch.equal(row[..., :used], c['off'][..., :used])
    got = run_kernels(x, row.to(DEV), g_cols, prior, relu_x, modulated)
    assert torch.equal(got['cols'], want['cols'])
    assert got['g_off'].shape == (N, H, W, ld) and got['g_off'].is_contiguous()
    assert torch.equal(got['g_off'][..., :used], want['g_off'][..., :used]) and float(got['g_off'][..., :used].abs().max()) > 0
    assert not got['g_off'][..., used:].any() and not want['g_off'][..., used:].any()
    for v in VARIANTS:
        assert torch.equal(got[v], want[v]), v
    # the reference once more, so that equal bits are not equal mistakes
    assert rel(got['cols'], c['r64']['cols']) <= floor_and_bar(c['r32']['cols'], c['r64']['cols'])[1]
    assert rel(got[(False, False)], c['r64']['gx']) <= floor_and_bar(c['r32']['gx'], c['r64']['gx'])[1]


# ---- the composed layer ------------------------------------------------------------------------------------------------------------------
from chainer_maskrcnn.nn import core                                              # noqa: E402
from chainer_maskrcnn.nn.core import DeformConv, ParamStore                        # noqa: E402
from chainer_maskrcnn._hip import nn as hnn                                        # noqa: E402
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import DEFAULT_GEMM_ARITHMETIC, select_gemm_arithmetic      # noqa: E402


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
@pytest.mark.parametrize('shape,modulated,kind', KERNEL_CASES + COMPOSED_WIDE_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_composed_layer_with_prescribed_offsets(shape, modulated, kind, arith):
    """The small shapes, and the widths of res3 / res4 / res5 on the same map: GEMMs over K = 1152 / 2304 / 4608, the depth of the shipped
    layers; on zero offsets the plain 3x3 layer of the same depth stands beside the float64 reference."""
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
from tests import step_harness                                                                   # noqa: E402

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


FULL_WIDTH = dict(stages=(1, 1, 1, 1), width_div=1)


@pytest.mark.parametrize('frozen', [False, True], ids=['batch_statistics', 'frozen_bn'])
@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
def test_deformable_blocks_inside_the_fpn(modulated, frozen):
    _blocks_inside_the_fpn(modulated, frozen, SHRINK, (2, 96, 128), (32, 64, 128))


def test_deformable_blocks_inside_the_full_width_fpn():
    """One block per stage at the widths the model ships with, v2, batch statistics, on a 2 x 64 x 96 image: res3 8 x 12 at 128 channels,
    res4 4 x 6 at 256, res5 2 x 3 at 512."""
    recs = _blocks_inside_the_fpn(True, False, FULL_WIDTH, (2, 64, 96), (128, 256, 512))
    assert [tuple(r['x'].shape) for r in recs] == [(2, 8, 12, 128), (2, 4, 6, 256), (2, 2, 3, 512)]


def _blocks_inside_the_fpn(modulated, frozen, net, image, widths):
    ext = FeaturePyramidNetwork(dcn_stages=ALL_STAGES, dcn_modulated=modulated, **net)
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
    img = torch.randn(tuple(image) + (4,), generator=g)
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
    assert [r['x'].shape[3] for r in recs] == list(widths)
    return recs


# ---- the whole model -------------------------------------------------------------------------------------------------------------------------
_build, _batch, _step = functools.partial(step_harness.build, SHRINK, mask_rows='positives'), step_harness.batch, step_harness.step


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
        step_harness.seed(chain)
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
