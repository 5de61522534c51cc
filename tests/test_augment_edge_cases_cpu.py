"""Every case of tests/augment_edge_cases.py is what it is named for - block counts, where the block boundaries fall, which ballot round
each kept or dropped candidate sits in, which byte values are present - asserted from plain arithmetic and from the NumPy rules
(resize_nearest + tight boxes; augment.copy_paste_batch), on any machine.  A case that misses its path fails HERE instead of silently
weakening tests/test_augment_edges_gpu.py.  The NumPy results are computed once per case (the builders are cached)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

from tests import augment_edge_cases as cases  # noqa: E402
from tests.augment_edge_cases import (BALLOT_CANVAS, BALLOT_DROPPED, BALLOT_GS, CANVASES, CANVAS_IDS, NT, WAVE, ballot_round,  # noqa: E402
                                      block_start, blocks, blocks_of, cp_candidates, exits_early, np_copy_paste, np_lsj, threads, wq)


def test_the_module_restates_the_constants_of_the_kernel_files():
    csrc = os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc')
    for name in ('augment.hip', 'copy_paste.hip'):
        src = open(os.path.join(csrc, name)).read()
        assert int(re.search(r'constexpr int NT = (\d+);', src).group(1)) == NT, name
        assert 'wq = (dst_w + 15) / 16' in src or 'wq = (W + 15) / 16' in src
        assert 'base += kWave' in src                                         # a ballot round is one wave of candidates
    assert int(re.search(r'constexpr int kWave = (\d+);', open(os.path.join(csrc, 'common.h')).read()).group(1)) == WAVE
    header = open(os.path.join(ROOT, 'include', 'mrcnn_hip.h')).read()
    assert int(re.search(r'#define MRCNN_RESIZE_BATCH_MAX (\d+)', header).group(1)) == cases.BATCH_MAX
    assert 'base += NT' in open(os.path.join(csrc, 'copy_paste.hip')).read()  # a pass of k_cp_compose stages NT rows


def test_the_canvases_leave_the_single_block_regime():
    for H, W in cases.OLD_CANVASES:
        assert blocks(H, W) == 1                                              # what the older GPU tests reach
    assert [wq(W) for _, W in CANVASES] == [8, 13, 13]
    assert [threads(H, W) for H, W in CANVASES] == [1024, 1300, 1300]
    assert [blocks(H, W) for H, W in CANVASES] == [4, 6, 6]
    assert [block_start(b, 128) for b in range(4)] == [(0, 0), (32, 0), (64, 0), (96, 0)]           # blocks of exactly 32 rows
    assert block_start(1, 208) == (19, 9) and block_start(5, 208) == (98, 6) and 1300 - 5 * NT == 20   # a split row; a partly idle block
    assert all(block_start(b, 208)[1] for b in range(1, 6)) and NT % 13 != 0                         # every boundary is inside a row
    assert [cases.mask_rows_vectorised(W) for _, W in CANVASES] == [True, True, False]
    assert [cases.image_rows_vectorised(W) for _, W in CANVASES] == [True, True, True] and 200 % 16 == 8
    assert not any(cases.image_rows_vectorised(W) for _, W in cases.OLD_CANVASES[1:])


# ---- large-scale jitter ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('canvas', CANVASES, ids=CANVAS_IDS)
def test_box_extremes_lie_in_different_blocks(canvas):
    H, W = canvas
    nb = blocks(H, W)
    batch = cases.extremes_case(canvas, 0)
    m, flip, geo = batch[0]
    assert geo == (H, W, 0, 0, H, W) and flip == 0
    assert blocks_of(m[0]) == [0, nb - 1] and m[0, 0, W - 1] and m[0, H - 1, 0]
    assert blocks_of(m[1]) == [nb - 1] and np.count_nonzero(m[1]) == 1 and m[1, H - 1, W - 1] == 255
    assert blocks_of(m[2]) == list(range(nb)) and np.count_nonzero(m[2]) == nb
    assert blocks_of(m[3]) == [0, 1] and blocks_of(m[4]) == [nb - 2, nb - 1]
    ys, xs = np.nonzero(m[3])
    if block_start(1, W)[1]:                                                  # one row, its first and last chunk, on either side of the boundary
        assert len(set(ys)) == 1 and sorted(x // 16 for x in xs) == [0, wq(W) - 1]
    else:                                                                     # the last thread of block 0 and the first of block 1
        assert [y * wq(W) + x // 16 for y, x in zip(ys, xs)] == [NT - 1, NT]
    want = np_lsj(batch, 5, canvas)
    np.testing.assert_array_equal(want['bboxes'][0, 0], [0, 0, H, W])         # right only if the maxima of the first and last block meet
    np.testing.assert_array_equal(want['bboxes'][0, 1], [H - 1, W - 1, H, W])
    assert want['gather'][0].tolist() == [0, 1, 2, 3, 4] and (want['labels'][1] >= 0).sum() == 3
    # the mirrored batch stores mirrored sources: the crop sees the same layout
    flipped = cases.extremes_case(canvas, 1)
    np.testing.assert_array_equal(flipped[0][0][:, :, ::-1], m)
    for k in ('bboxes', 'gather', 'masks'):
        np.testing.assert_array_equal(np_lsj(flipped, 5, canvas)[k], want[k])


@pytest.mark.parametrize('name', sorted(cases.WINDOW_CASES))
def test_window_shorter_than_the_canvas(name):
    canvas, ch = cases.WINDOW_CASES[name]
    H, W = canvas
    batch = cases.window_case(name, 0)
    m, _, geo = batch[0]
    assert geo[4] == ch and geo[0] - geo[2] > ch                              # rows of the virtual resize below the window
    early = [exits_early(b, W, ch) for b in range(blocks(H, W))]
    want = np_lsj(batch, len(m), canvas)
    seen = [blocks_of(p) for p in want['masks'][0]]
    if name == 'ch40_128x128':
        assert early == [False, False, True, True] and block_start(1, W)[0] < ch - 1 < block_start(2, W)[0]      # block 1 straddles row 39 | 40
        assert want['kept'][0] == [0, 2, 5, 6] and seen[:4] == [[0, 1], [0, 1], [1], [1]]
        np.testing.assert_array_equal(want['bboxes'][0, :4], [[0, 0, 40, 100], [30, 20, 40, 41], [39, 99, 40, 100], [33, 50, 37, 71]])
        assert sorted(set(want['masks'].reshape(-1))) == [0, 1, 2, 128, 255]
    else:
        assert early == [False, False, True, True, True, True] and block_start(1, W) == (ch - 1, 9)             # the last window row is the split row
        assert want['kept'][0] == [0, 1, 3, 4] and seen[:4] == [[0, 1], [1], [0], [0, 1]]
        np.testing.assert_array_equal(want['bboxes'][0, :4], [[19, 0, 20, 208], [19, 150, 20, 151], [0, 100, 20, 144], [15, 130, 20, 161]])
    assert not want['masks'][0, :, ch:].any() and want['masks'][0, :, ch - 1].any()
    dropped = sorted(set(range(len(m))) - set(want['kept'][0]))
    assert dropped and all(m[g].any() for g in dropped)                       # dropped by the window, not empty to begin with


def test_ballot_case_spans_three_rounds():
    batch = cases.ballot_case(0)
    assert [b[0].shape[0] for b in batch] == [130, 65, 0] and blocks(*BALLOT_CANVAS) == 2
    assert 3 * 130 * BALLOT_CANVAS[0] * BALLOT_CANVAS[1] <= 3 * 80 * 128 * 128
    assert sorted({ballot_round(g) for g in BALLOT_DROPPED}) == [0, 1, 2] and ballot_round(129) == 2
    full = np_lsj(batch, 130, BALLOT_CANVAS)
    kept = full['kept']
    assert kept[0] == [g for g in range(130) if g not in BALLOT_DROPPED] and kept[1] == [64] and kept[2] == []
    per_round = [sum(ballot_round(g) == r for g in kept[0]) for r in range(3)]
    assert per_round == [63, 61, 1]
    # where the truncation falls: no row is cut off; inside round 1; two rows into, one row into and in front of round 1
    assert BALLOT_GS == [130, 100, 65, 64, 63] and len(kept[0]) == 125
    for G, last_round, rows_of_round_1 in ((130, 2, 61), (100, 1, 37), (65, 1, 2), (64, 1, 1), (63, 0, 0)):
        want = np_lsj(batch, G, BALLOT_CANVAS)
        table = want['gather'][0][want['gather'][0] >= 0]
        assert len(table) == min(G, 125) and ballot_round(int(table[-1])) == last_round
        assert sum(ballot_round(int(g)) == 1 for g in table) == rows_of_round_1
        assert want['gather'][1].tolist() == [64] + [-1] * (G - 1) and want['labels'][1, 0] == 2064      # lane 0 of round 1, nothing kept before
        assert (want['gather'][2] == -1).all()
    cut = [g for g in kept[0] if g % 10 == 9]
    assert cut and all(full['bboxes'][0, kept[0].index(g), 0] == 0 and full['bboxes'][0, kept[0].index(g), 2] == 8 for g in cut)


@pytest.mark.parametrize('crop', [False, True], ids=['plain', 'crop'])
def test_a_full_batch_of_different_examples(crop):
    imgs, batch = cases.many_case(crop, 0)
    assert len(batch) == cases.BATCH_MAX == 32
    geos = [cases.many_geometry(n, crop) for n in range(32)]
    assert len(set(geos)) == 32 and len({g[4] for g in geos}) >= 28
    H, W, flip, count, (oh, ow, y0, x0, ch, cw) = geos[-1]                    # the last descriptor does something
    assert count == 3 and flip == 1
    if crop:
        assert oh > ch == 16 and ow > cw == 32 and y0 > 0 and x0 > 0
        assert 32 * 48 == 1536                                                # bytes of descriptors in the kernel's arguments
    want = np_lsj(batch, 3, cases.MANY_CANVAS)
    assert want['masks'][31].any() and len(want['kept'][31]) == 3
    assert cases.np_images([(i, f, g) for i, (_, f, g) in zip(imgs, batch)], cases.MANY_CANVAS)[31].any()


# ---- Copy-Paste -----------------------------------------------------------------------------------------------------------------------------
def _labels_by_state(case):
    """The labels the rule keeps, from cp_candidates: what copy_paste_batch must return with room for every row."""
    batch, _, _, _ = case
    labels = batch['labels']
    N, G = labels.shape
    state = cp_candidates(case)
    return state, [[int(labels[n, c] if c < G else labels[(n + 1) % N, c - G]) for c in np.flatnonzero(state[n] == 1)] for n in range(N)]


def _consistent(case):
    state, kept = _labels_by_state(case)
    out = np_copy_paste(case, None)
    for n, l in enumerate(kept):
        assert out['labels'][n][out['labels'][n] >= 0].tolist() == l
    return state, out


@pytest.mark.parametrize('N', [2, 3])
@pytest.mark.parametrize('canvas', CANVASES, ids=CANVAS_IDS)
def test_multi_block_copy_paste_case(canvas, N):
    H, W = canvas
    nb = blocks(H, W)
    case = cases.cp_multiblock(canvas, N)
    batch, gather, sel, receive = case
    state, out = _consistent(case)
    assert batch['masks'].shape == (N, cases.MULTI_G, H, W) and receive.tolist() == [1, 1, 0][:N]
    assert state[0].tolist() == [1, 0, 1, 1, -1, 1, 1, -1, 1, -1]
    left = np.where(batch['masks'][1, [0, 1, 3]].any(0), 0, batch['masks'][0])      # example 0's rows under what example 1 pastes
    b = blocks_of(left[0])
    assert len(b) == 2 and b[0] == 0 and b[1] - b[0] >= 3                     # cut: what is left lies in non-adjacent blocks
    np.testing.assert_array_equal(out['bboxes'][0, 0], [5, 40, H - 5, 61])    # its box needs both
    assert batch['masks'][0, 1].any() and not left[1].any()                   # covered entirely
    assert blocks_of(left[2]) == [nb - 1] and np.count_nonzero(left[2]) == 2  # the last pixels are in the last block ...
    assert (threads(H, W) % NT != 0) == (wq(W) == 13)                         # ... which is partly idle on the 13-chunk canvases
    np.testing.assert_array_equal(out['bboxes'][0, 1], [H - 2, W - 1, H, W])
    assert out['labels'][0].tolist()[:6] == [1, 3, 4, 5, 6, 8]
    if N == 2:                                                                # each example is the other's partner
        assert state[1].tolist()[5:] == [1, -1, -1, 1, -1] and out['labels'][1].tolist()[:6] == [5, 6, 7, 8, 1, 4]
        assert (batch['masks'][1, 0] * batch['masks'][0, 0]).any()            # and example 0's tall row cuts example 1's cover
    else:
        assert (state[2][cases.MULTI_G:] == -1).all() and (out['imgs'][2] == batch['imgs'][2]).all()


@pytest.mark.parametrize('G', cases.WAVE_GS)
def test_candidates_past_one_wave(G):
    case = cases.cp_waves(G)
    state, out = _consistent(case)
    rounds = -(-2 * G // WAVE)
    assert rounds == {40: 2, 70: 3}[G] and case[0]['masks'].nbytes <= 3 * 80 * 128 * 128
    kept = (state == 1).sum(1)
    g_outs = cases.wave_g_outs(G)
    assert kept.max() + 1 in g_outs and 3 * max(g_outs) * 128 * 128 <= 3 * 80 * 128 * 128     # a G_out past every kept count
    assert {33, 64, 65, int(kept[0])} <= set(g_outs)
    for n in range(3):
        by_round = [state[n, r * WAVE:(r + 1) * WAVE] for r in range(rounds)]
        own_rounds = -(-(G - 4) // WAVE)
        assert all((s[:max(0, G - r * WAVE)] == 0).any() for r, s in enumerate(by_round[:own_rounds])), n     # own rows dropped in every round that has some
        picked = [(state[n, max(G, r * WAVE):(r + 1) * WAVE] == 1).sum() for r in range(rounds)]
        assert all(p > 0 for p in picked[(G // WAVE):]), (n, picked)                                           # partner rows picked in every round that has some
        assert any((s == 1).any() and (s == 0).any() for s in by_round)
    if G == 70:
        assert kept[0] > 65 and (state[0, :64] == 1).sum() < 64 < (state[0, :128] == 1).sum()                # G_out = 64 | 65 cut inside round 1
        assert (state[0, :64] == 1).sum() > 33                                                              # 33 cuts inside round 0
        assert [np.flatnonzero(state[0, :G] == 0).tolist()] == [[4, 19, 34, 49, 64]]
    else:
        assert kept.max() < 64                                                                              # 64 and 65: rows behind the kept ones
    # a cut row whose box shrinks: own 4 x 4 under a picked top half
    own = np.flatnonzero((state[0, :G] == 1))
    shrunk = [g for k, g in enumerate(own) if (out['bboxes'][0, k] != case[0]['bboxes'][0, g]).any()]
    assert shrunk and all(g % 3 == 0 for g in shrunk)
    # the offer goes through the gather table: original 5 is missing, so row j >= 5 is original j + 1
    assert case[1][0, 4:7].tolist() == [4, 6, 7] and case[2].shape == (3, G + 1)


def test_more_rows_than_one_pass_of_picks():
    case = cases.cp_many_rows()
    batch, gather, sel, receive = case
    state, out = _consistent(case)
    G = cases.MANY_ROWS_G
    assert G == NT + 1 and batch['masks'].shape == (2, G) + cases.MANY_ROWS_CANVAS
    assert np.flatnonzero(state[0, G:] >= 0).tolist() == [256]                # example 0 takes row 256 alone: the second pass' only row
    assert np.flatnonzero(state[1, G:] >= 0).tolist() == [3, 100, 255, 256]   # example 1: both passes
    assert not (batch['masks'][1, 256] == batch['masks'][1, 0]).all()         # (row 0 in its place would show)
    kept = (state == 1).sum(1)
    assert kept.tolist() == [(state[0, :G] == 1).sum() + 1, (state[1, :G] == 1).sum() + 4] and np.argwhere(state[:, :G] == 0).tolist() == [[0, 200], [1, 10]]
    assert kept.max() < cases.MANY_ROWS_G_OUT and -(-2 * G // WAVE) == 9


@pytest.mark.parametrize('canvas', [CANVASES[0], CANVASES[2]], ids=[CANVAS_IDS[0], CANVAS_IDS[2]])
def test_byte_values_reach_every_lane(canvas):
    case = cases.cp_byte_values(canvas)
    batch = case[0]
    state, out = _consistent(case)
    assert (state == cp_candidates(cases.cp_multiblock(canvas, 3))).all()
    for n in (0, 1):                                                          # own (0) and pasted (1) masks
        for lane in range(4):
            v = set(batch['masks'][n][:, :, lane::4].reshape(-1)) - {0}
            assert v == {1, 2, 128, 255}, (n, lane, v)                        # with and without bit 7, with and without bit 0
    assert set(out['masks'][0].reshape(-1)) == {0, 1, 2, 128, 255}            # the rule keeps the byte value
    plain = np_copy_paste(cases.cp_multiblock(canvas, 3), None)
    np.testing.assert_array_equal(out['masks'] != 0, plain['masks'] != 0)
    np.testing.assert_array_equal(out['imgs'], plain['imgs'])
    np.testing.assert_array_equal(out['bboxes'], plain['bboxes'])


@pytest.mark.parametrize('kind', ['receive', 'sel'])
def test_nothing_pasted_case(kind):
    case = cases.cp_no_paste(kind)
    batch, gather, sel, receive = case
    state, out = _consistent(case)
    assert (state[:, cases.MULTI_G:] == -1).all() and not (receive.any() and sel.any())
    assert blocks(*batch['masks'].shape[2:]) == 6
    np.testing.assert_array_equal(out['imgs'], batch['imgs'])
    np.testing.assert_array_equal(out['masks'][:2], batch['masks'][:2, :4])
    assert batch['labels'][2].tolist() == [9, 10, 11, -1, -1] and out['labels'][2].tolist() == [9, 11, -1, -1]      # compacted
    np.testing.assert_array_equal(out['masks'][2, 1], batch['masks'][2, 2])
