"""The cases that take the Mask Scoring R-CNN kernels (csrc/maskiou.hip) away from N = 2, G = 4, 28 x 28 logits
and one grid pass, and the kernels' thread maps restated as plain arithmetic.  Imports without the library or a device:
tests/test_maskiou_edge_cases_cpu.py holds every case to the path it is named for, tests/test_maskiou_edges_gpu.py compares kernel and
reference (tests/maskiou_reference.py) on them.

A helper of the tests, not a test and not part of the product."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskiou_reference as mr            # noqa: E402

# ---- the thread maps ------------------------------------------------------------------------------------------------------------------------
NT = 256                        # threads of k_mask_area and of the elementwise and loss kernels
TB = 512                        # threads of k_maskiou_target; masks a trailing workgroup of it sums
MI_CHUNKS = 32                  # workgroups per mask of k_mask_area
LOSS_BLOCKS = 1024              # workgroups of the loss kernels (grid_for)
LINES_PER_TRIP = TB // 16       # a line of the crop rectangle per 16 lanes


def cdiv(a, b):
    return -(-a // b)


def area_split(addr, HW):
    """(head, nvec, tail) of a mask of HW bytes at byte address ``addr``: the bytes in front of the first 16-byte boundary, the aligned
    16-byte vectors, the bytes behind the last."""
    head = min((16 - addr % 16) % 16, HW)
    nvec = (HW - head) // 16
    return head, nvec, HW - head - 16 * nvec


def chunk_shares(nvec):
    """[(v0, v1)] the vectors of every one of the MI_CHUNKS workgroups of a mask."""
    per = cdiv(nvec, MI_CHUNKS)
    return [(min(c * per, nvec), min(min(c * per, nvec) + per, nvec)) for c in range(MI_CHUNKS)]


def empty_chunks(nvec):
    return sum(1 for a, b in chunk_shares(nvec) if a == b)


def sum_workgroups(N, G):
    """Trailing workgroups of k_maskiou_target that add the area partials."""
    return cdiv(N * G, TB)


def line_trips(h):
    return cdiv(h, LINES_PER_TRIP)


def logit_trips(mask_size):
    return cdiv(mask_size * mask_size, TB)


def loss_grid(n):
    return max(1, min(cdiv(n, NT), LOSS_BLOCKS))


def loss_trips(n):
    return cdiv(n, loss_grid(n) * NT)


# ---- the area pass --------------------------------------------------------------------------------------------------------------------------
MANY = (27, 19, 5, 5, 0)
# (N, G, H, W, byte offset of the mask buffer from a 16-byte boundary): H * W = 1, 9, 16, 96, 544
AREA_CASES = (MANY, (3, 3, 1, 1, 0), (3, 3, 3, 3, 0), (3, 3, 4, 4, 0), (3, 3, 8, 12, 3), (3, 3, 16, 34, 3))
AREA_IDS = ['%dx%d masks of %dx%d at +%d' % c for c in AREA_CASES]


@functools.lru_cache(maxsize=None)
def area_case(N, G, H, W, offset):
    return mr.area_case(N, G, H, W)


# ---- the target pass ------------------------------------------------------------------------------------------------------------------------
MASK_SIZES = (1, 14, 23)
PAD_ROW = 15                    # the row of every image of mr.crop_case whose label selects a padding channel


@functools.lru_cache(maxsize=None)
def crop_case(mask_size):
    return mr.crop_case(mask_size)


# ---- input assembly, loss, rescoring --------------------------------------------------------------------------------------------------------
INPUT_P, INPUT_C, N_FG = (1, 7), (4, 256), 3
INPUT_LABEL = np.array([1, N_FG, 0, -1, N_FG + 1, 2], np.int32)         # first and last class, background, padding row, a PADDING CHANNEL


def input_case(P, C):
    rs = np.random.RandomState(P * 1000 + C)
    Rm, Cp = len(INPUT_LABEL), mr.pad32(N_FG)
    logit = (rs.standard_normal((Rm, 2 * P, 2 * P, Cp)) * 3).astype(np.float32)
    logit[logit == 0] = 1.0
    return dict(feat=rs.standard_normal((Rm, P, P, C)).astype(np.float32), mask_out=logit, label=INPUT_LABEL.copy(), cin_p=C + 4,
                g_in=rs.standard_normal((Rm, P, P, C + 4)).astype(np.float32), g_pool=rs.standard_normal((Rm, P, P, C)).astype(np.float32))


L2_ROWS, L2_LD = 270000, 4


@functools.lru_cache(maxsize=None)
def l2_case():
    """Rm > 1024 * 256 rows of ld = 4 columns, three of them classes: labels 0 .. 4, so label 4 selects the padding column."""
    rs = np.random.RandomState(27)
    pred = rs.standard_normal((L2_ROWS, L2_LD)).astype(np.float32)
    tgt = np.where(rs.rand(L2_ROWS) < 0.6, rs.rand(L2_ROWS), 0.0).astype(np.float32)
    label = rs.randint(0, N_FG + 2, L2_ROWS).astype(np.int32)
    label[-1], tgt[-1] = N_FG, 0.5              # the last row, in the second trip, counts
    label[-2], tgt[-2] = N_FG + 1, 0.5          # and its neighbour selects the padding column
    return dict(pred=pred, target=tgt, label=label)


RESCORE_D, RESCORE_LD, RESCORE_CH = 257, 8, 5


def rescore_case():
    rs = np.random.RandomState(3)
    pred = (rs.standard_normal((RESCORE_D, RESCORE_LD)) * 0.8 + 0.5).astype(np.float32)
    label = rs.randint(0, RESCORE_CH, RESCORE_D).astype(np.int32)
    label[:4] = (-1, RESCORE_LD, RESCORE_CH, RESCORE_LD - 1)    # no label, past the columns, the first and the last padding column
    label[-1] = RESCORE_CH - 1                                  # detection 256: the second workgroup
    pred[:4] = 0.5
    pred[-1] = 0.25
    return dict(score=(rs.rand(RESCORE_D) + 0.1).astype(np.float32), pred=pred, label=label)
