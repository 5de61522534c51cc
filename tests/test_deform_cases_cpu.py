"""Every case of tests/deform_cases.py reaches the tier of csrc/deform.hip it is named for - asserted from tests/deform_reference.list_lengths
and plain arithmetic, on any machine.  A case that misses its tier fails HERE instead of silently weakening tests/test_deform_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_cases as cases  # noqa: E402
import deform_reference as dr  # noqa: E402
from deform_cases import LIST_MAX, LONG_CHUNK, LONG_GRID, LONG_SHAPE, LONG_WAVES, RANK_MAX, ROUND, SCAN_T, SHAPES, make_offsets  # noqa: E402


def lengths(shape, kind, modulated=False):
    return dr.list_lengths(make_offsets(kind, shape, modulated, cases.offset_seed(shape)), shape).reshape(-1)


def tiers(f):
    """(lists ordered by rank, lists ordered by the network in LDS, lists of the workgroup kernel)."""
    return int(((f > 0) & (f <= RANK_MAX)).sum()), int(((f > RANK_MAX) & (f <= LIST_MAX)).sum()), int((f > LIST_MAX).sum())


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


def test_the_module_restates_the_constants_of_the_kernel_file():
    """The tier constants are csrc/deform.hip's, read from its text."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'chainer-maskrcnn_amd', 'csrc', 'deform.hip')).read()
    for name, want in (('LIST_MAX', LIST_MAX), ('LONG_T', cases.LONG_T), ('LONG_CHUNK', LONG_CHUNK), ('LONG_GRID', LONG_GRID), ('SCAN_T', SCAN_T),
                       ('C_MAX', cases.C_MAX)):
        assert int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1)) == want, name
    assert 'C / 4 <= 32' in src and 'lane + 64 < C4' in src and 'n <= 64' in src


# ---- the channel tiers ---------------------------------------------------------------------------------------------------------------------------
# C: GL, (most, fewest) trips of the channel loop, idle lanes of a group, (lanes with the first, with the second accumulator), live threads
# of the long-list kernel
WIDTH_TIERS = {128: (32, (1, 1), 0, (32, 0), 128),          # the last <32> width, every lane one trip: res3
               132: (64, (1, 0), 31, (33, 0), 132),         # the first <64> width
               256: (64, (1, 1), 0, (64, 0), 256),          # a full wave, one trip, no second accumulator yet: res4
               260: (64, (2, 1), 0, (64, 1), 260),          # lane 0 alone has the second accumulator
               512: (64, (2, 2), 0, (64, 64), 512),         # C_MAX: both accumulators in every lane, every long-kernel thread live: res5
               516: (64, (3, 2), 0, None, None),
               1024: (64, (4, 4), 0, None, None)}


@pytest.mark.parametrize('C', cases.WIDTHS + cases.OVER_WIDTHS)
def test_width_reaches_its_channel_tier(C):
    GL, trips, idle, acc, live = WIDTH_TIERS[C]
    assert C % 4 == 0 and cases.group_lanes(C) == GL and cases.channel_trips(C) == trips and cases.idle_lanes(C) == idle
    if C in cases.OVER_WIDTHS:
        assert C > cases.C_MAX
        return
    assert C <= cases.C_MAX and cases.accumulator_lanes(C) == acc and cases.long_live_threads(C) == live
    # the slices a wide call is compared with cover every channel and run in the tier SHAPES pins
    starts = cases.slice_starts(C)
    covered = torch.zeros(C, dtype=torch.bool)
    for s in starts:
        assert 0 <= s and s + cases.SLICE <= C
        covered[s:s + cases.SLICE] = True
    assert covered.all() and any(s[3] == cases.SLICE for s in SHAPES)


def test_widths_sit_on_both_sides_of_every_branch_on_the_channel_count():
    gl = [cases.group_lanes(C) for C in cases.WIDTHS]
    assert cases.group_lanes(128) == 32 and cases.group_lanes(132) == 64 and set(gl) == {32, 64}
    assert cases.accumulator_lanes(256)[1] == 0 and cases.accumulator_lanes(260)[1] == 1 and cases.accumulator_lanes(512)[1] == 64
    assert max(cases.WIDTHS) == cases.C_MAX and min(cases.OVER_WIDTHS) == cases.C_MAX + 4
    assert {cases.channel_trips(C)[0] for C in cases.WIDTHS + cases.OVER_WIDTHS} == {1, 2, 3, 4}


@pytest.mark.parametrize('C', cases.WIDTHS + cases.OVER_WIDTHS)
def test_width_sets_reach_the_three_list_tiers(C):
    """Every width sees lists ordered by rank, lists ordered in LDS beside short ones and the workgroup kernel."""
    shape = cases.WIDTH_MAP + (C,)
    for kind in ('b_integer', 'c_fractional'):
        f = lengths(shape, kind)
        assert 0 < int(f.max()) <= RANK_MAX and tiers(f)[0] >= 69, (kind, f.max())
    d = lengths(shape, 'd_one_cell')
    assert tiers(d) == (0, 0, 2) and [int(i) for i in d.nonzero().reshape(-1)] == [34, 69] and int(d.max()) == 9 * 5 * 7 == 315 <= ROUND
    f = lengths(shape, 'f_few_cells')
    assert tiers(f) == (54, 16, 0) and RANK_MAX < int(f[f > RANK_MAX].min()) and int(f.max()) <= 121
    if C == 256:
        assert int(f.max()) == 119


def test_the_wide_long_case_takes_two_rounds_of_chunks_with_every_thread_live():
    shape, kind = cases.WIDE_LONG
    f = lengths(shape, kind)
    assert shape[3] == cases.C_MAX == cases.long_live_threads(shape[3]) == cases.LONG_T
    assert tiers(f) == (0, 0, 16) and int(f.max()) == int(f[f > 0].min()) == 1296 and ROUND < 1296 <= 2 * ROUND


# ---- the scan --------------------------------------------------------------------------------------------------------------------------------------
# map: P, (per, threads with a full range, with a partial one, idle)
SCAN_TIERS = {(1, 32, 32, 32): (1024, (1, 1024, 0, 0)),
              (1, 25, 41, 32): (1025, (2, 512, 1, 511)),
              (1, 33, 32, 32): (1056, (2, 528, 0, 496)),
              (2, 40, 30, 32): (2400, (3, 800, 0, 224))}


@pytest.mark.parametrize('shape,kinds', cases.SCAN_CASES, ids=str)
def test_scan_case_reaches_its_layout(shape, kinds):
    P, layout = SCAN_TIERS[shape]
    assert shape[0] * shape[1] * shape[2] == P and shape[3] == 32 and cases.scan_layout(P) == layout
    per, full, partial, idle = layout
    assert full * per + (P - full * per if partial else 0) == P and full + partial + idle == SCAN_T
    assert 'c_fractional' in kinds
    f = lengths(shape, 'c_fractional')
    assert tiers(f) == (P, 0, 0)                                 # every destination has a list: no thread scans zeros only


def test_scan_cases_cover_one_two_and_three_destinations_per_thread():
    per = [cases.scan_layout(s[0] * s[1] * s[2])[0] for s, _ in cases.SCAN_CASES]
    assert sorted(set(per)) == [1, 2, 3]
    assert cases.scan_layout(1024) == (1, SCAN_T, 0, 0) and cases.scan_layout(1025)[2] == 1       # the last of 513 threads holds one destination
    assert all(cases.scan_layout(s[0] * s[1] * s[2])[0] == 1 for s in SHAPES + [LONG_SHAPE])      # what the older cases reach


def test_long_lists_spread_over_the_scan_threads():
    """(1,33,32,32) with 16 targets: 64 long lists, more than the workgroups of the long-list kernel, whose ids are continued from the
    prefixes of many scan threads."""
    shape = (1, 33, 32, 32)
    assert 'g_targets16' in dict(cases.SCAN_CASES)[shape]
    f = lengths(shape, 'g_targets16')
    P = 33 * 32
    assert tiers(f) == (0, 0, 64) and 64 > LONG_GRID and int(f.max()) == 594 <= ROUND and int(f[f > 0].min()) > LIST_MAX
    where = [int(i) for i in (f > LIST_MAX).nonzero().reshape(-1)]
    threads = [cases.scan_thread_of(d, P) for d in where]
    assert len(set(threads)) == 32 and all(threads.count(t) == 2 for t in set(threads))          # two per thread: both destinations of its range
    assert min(threads) > 0 and max(threads) < cases.scan_layout(P)[1] - 1


def test_the_two_image_map_has_long_lists_at_both_ends_of_the_scan():
    shape = cases.TWO_IMAGE_SHAPE
    kinds = dict(cases.SCAN_CASES)[shape]
    assert set(kinds) == {'c_fractional', 'd_one_cell', 'f_few_cells'} and shape[0] == 2
    P, per = 2400, 3
    f = lengths(shape, 'f_few_cells')
    where = [int(i) for i in (f > LIST_MAX).nonzero().reshape(-1)]
    assert where == [0, 1, 30, 31, 1168, 1169, 1198, 1199, 1200, 1201, 1230, 1231, 2368, 2369, 2398, 2399]
    assert int(f.max()) == 3613 and -(-3613 // ROUND) == 4 and tiers(f)[1] == 0 and tiers(f)[0] == 2382
    threads = [cases.scan_thread_of(d, P) for d in where]
    assert threads[0] == 0 and threads[-1] == cases.scan_layout(P)[1] - 1 == 799                   # the first and the last busy thread
    assert cases.scan_thread_of(1199, P) == 399 and cases.scan_thread_of(1200, P) == 400          # the images meet between two threads
    d = lengths(shape, 'd_one_cell')
    assert [int(i) for i in d.nonzero().reshape(-1)] == [1199, 2399] and int(d.max()) == 9 * 40 * 30 == 10800 and -(-10800 // ROUND) == 11


# ---- the offset row strides ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
def test_stride_cases(modulated):
    used = cases.used_channels(modulated)
    lds = cases.STRIDES[modulated]
    assert lds[0] == used and (lds[0] * 4) % 16 != 0                      # no padded channel; rows not 16-byte aligned
    assert used < lds[1] < cases.LD < lds[2] and lds[1] % 4 == 0          # a few padded channels on aligned rows; a row wider than LD
    shape = cases.STRIDE_SHAPE
    assert shape[3] == cases.SLICE
    for kind in cases.STRIDE_SETS:
        base = make_offsets(kind, shape, modulated, cases.offset_seed(shape))
        for ld in lds:
            off = make_offsets(kind, shape, modulated, cases.offset_seed(shape), ld=ld)
            assert off.shape == shape[:3] + (ld,) and torch.equal(off[..., :used], base[..., :used])
            assert (off[..., used:] == cases.PAD_FILL).all()
    assert tiers(lengths(shape, 'f_few_cells'))[1] == 16 and tiers(lengths(shape, 'c_fractional')) == (70, 0, 0)
