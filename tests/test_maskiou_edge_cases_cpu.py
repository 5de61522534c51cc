"""Every case of tests/maskiou_edge_cases.py is what it is named for - how a mask splits into head, vectors and tail, which chunks have
an empty share, how many trips the line and position loops take, which rows lose their class - asserted from the module's plain
arithmetic and from tests/maskiou_reference.py alone, on any machine.  A case that misses its path fails HERE instead of silently
weakening tests/test_maskiou_edges_gpu.py."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import maskiou_reference as mr  # noqa: E402
from tests import maskiou_edge_cases as cases  # noqa: E402

CSRC = os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc')


def test_the_module_restates_the_constants_of_the_kernel_file():
    src = open(os.path.join(CSRC, 'maskiou.hip')).read()
    loss = open(os.path.join(CSRC, 'loss_common.h')).read()
    assert int(re.search(r'constexpr int NT = (\d+);', loss).group(1)) == cases.NT
    assert int(re.search(r'constexpr int MAXB = (\d+);', loss).group(1)) == cases.LOSS_BLOCKS
    assert int(re.search(r'constexpr int MI_CHUNKS = (\d+);', src).group(1)) == cases.MI_CHUNKS
    assert int(re.search(r'constexpr int TB = (\d+);', src).group(1)) == cases.TB
    for text in ('y += TB / 16', 'p += TB', 'mrcnn::cdiv(N * G, TB)', 'const long long per = (nvec + MI_CHUNKS - 1) / MI_CHUNKS;'):
        assert text in src, text
    # the four kernels that read a label take n_channels and test the channel against it, not against the padded width
    for kernel in ('k_maskiou_target', 'k_maskiou_input_fwd', 'k_maskiou_l2', 'k_maskiou_rescore'):
        body = src[src.index('void ' + kernel + '('):]
        body = body[:body.index('\n}\n')]
        assert 'int n_channels' in body and 'ch < n_channels' in body and 'ch < Cp' not in body and 'ch < ld' not in body and 'ch >= ld' not in body, kernel


def test_what_the_older_cases_reach():
    # N = 2, G = 4, 28 x 28 logits, 37 x 45 and 64 x 64 masks: one summing workgroup, two full trips over the logits, chunks never empty
    assert cases.sum_workgroups(2, 4) == 1 and cases.logit_trips(28) == 2 and 28 * 28 >= cases.TB
    assert all(cases.area_split(a, hw)[1] >= 32 for hw in (37 * 45, 64 * 64) for a in range(16))
    assert cases.loss_trips(1500) == 1


@pytest.mark.parametrize('case', cases.AREA_CASES, ids=cases.AREA_IDS)
def test_area_cases(case):
    N, G, H, W, offset = case
    c = cases.area_case(*case)
    HW = H * W
    assert c['masks'].shape == (N, G, H, W)
    n_gt = c['n_gt']
    assert n_gt[0] == 0 and 0 < n_gt[1] < G and n_gt[N - 1] == G                               # n_gt below G
    assert all((c['masks'][i, n_gt[i]:] == 255).all() for i in range(N))                       # junk in the unused slots
    area = mr.mask_areas(c['masks'], n_gt)
    assert area[N - 1, G - 1] > 0 and not area[0].any() and not area[1, n_gt[1]:].any() and area.sum() > 0
    splits = [cases.area_split(offset + m * HW, HW) for m in range(N * G)]
    assert all(h + 16 * v + t == HW and h < 16 and t < 16 for h, v, t in splits)
    if case == cases.MANY:
        assert N * G == 513 and cases.sum_workgroups(N, G) == 2                                # mask 512: the second summing workgroup
        assert area.reshape(-1)[512] > 0
        assert {(offset + m * HW) % 16 for m in range(N * G)} == set(range(16))                # mask starts on every residue mod 16
    else:
        want = {1: 0, 9: 0, 16: 1, 96: 5, 544: 33}[HW]
        h, v, t = splits[0]
        assert v == want
        if HW < 16:
            assert all(s[1] == 0 for s in splits)                                               # no aligned vector at all
        if 0 < want < 32:
            assert cases.empty_chunks(want) == 32 - want                                        # chunks with an empty share
        if want == 33:
            shares = cases.chunk_shares(33)
            assert shares[0] == (0, 2) and shares[16] == (32, 33) and cases.empty_chunks(33) == 15
        if offset:
            assert h == 16 - offset and t > 0                                                   # a head and a tail, both counted by chunk 0


@pytest.mark.parametrize('mask_size', cases.MASK_SIZES)
def test_crop_cases(mask_size):
    c = cases.crop_case(mask_size)
    N, G, H, W = c['masks'].shape
    assert W % 2 == 1 and c['rows'] < c['n_sample'] and c['mask_out'].shape[1] == mask_size
    assert [cases.logit_trips(s) for s in cases.MASK_SIZES] == [1, 1, 2] and 14 * 14 < cases.TB and 23 * 23 % cases.TB
    seen = set()
    for j in range(15):
        y0, y1, x0, x1 = mr.crop_rect(c['sample_roi'][j], H, W)
        assert (y0, x0, y1 - y0, x1 - x0) == mr.crop_rects()[j] and y1 <= H and x1 <= W
        seen.add((x1 - x0, x0 % 16, y1 - y0))
    assert {(w, r) for w, r, _ in seen} == {(w, r) for w in (1, 15, 16, 17, 33) for r in (0, 1, 15)}
    assert {h for _, _, h in seen} == {1, 40} and [cases.line_trips(h) for h in (1, 40)] == [1, 2]
    counts = mr.target_counts(c)
    t32 = mr.target_from_counts(counts, np.float32)
    rows = c['rows']
    live = np.ones((N * rows,), bool)
    live[cases.PAD_ROW::rows] = False
    live[16::rows] = False
    assert (counts[live, 0] > 0).all() and (counts[live, 1] > 0).any() and (t32[live] > 0).any()
    # the row whose label selects a padding channel: no class, so zero counts and a zero target - although that channel, read as a
    # class, would give a positive one
    assert (c['label'][cases.PAD_ROW::rows] == c['n_fg'] + 1).all() and c['mask_out'].all()
    assert not counts[cases.PAD_ROW::rows].any() and not t32[cases.PAD_ROW::rows].any()
    as_class = mr.target_from_counts(mr.target_counts(dict(c, n_fg=c['n_fg'] + 1)), np.float32)
    assert (as_class[cases.PAD_ROW::rows] > 0).all() and np.array_equal(as_class[live], t32[live])


def test_input_loss_and_rescore_cases():
    for P in cases.INPUT_P:
        for C in cases.INPUT_C:
            c = cases.input_case(P, C)
            assert c['cin_p'] == C + 4 and c['mask_out'].shape == (6, 2 * P, 2 * P, 32) and c['mask_out'].all()
            w = mr.input_fwd(c['feat'], c['mask_out'], c['label'], c['cin_p'], n_channels=cases.N_FG)
            assert w[[0, 1, 5], :, :, C].all() and not w[[2, 3, 4], :, :, C].any() and not w[..., C + 1:].any()
            wide = mr.input_fwd(c['feat'], c['mask_out'], c['label'], c['cin_p'])
            assert wide[4, :, :, C].all()                               # what the padding channel would have put there
    c = cases.l2_case()
    assert len(c['label']) > 1024 * 256 and cases.loss_trips(cases.L2_ROWS) == 2 and cases.loss_trips(cases.L2_ROWS * cases.L2_LD) == 5
    loss, count, gx = mr.l2(c['pred'], c['target'], c['label'], n_channels=cases.N_FG)
    pad = c['label'] == cases.N_FG + 1
    assert (pad & (c['target'] > 0)).sum() > 1000 and not gx[pad].any() and gx[-1, cases.N_FG - 1] != 0 and not gx[-2].any()
    assert count == ((c['target'] > 0) & (c['label'] >= 1) & (c['label'] <= cases.N_FG)).sum()
    assert mr.l2(c['pred'], c['target'], c['label'])[1] > count         # read as a class, the padding column would count
    c = cases.rescore_case()
    w = mr.rescore(c['score'], c['pred'], c['label'], cases.RESCORE_CH)
    assert len(w) == 257 and not w[:4].any() and w[-1] == c['score'][-1] * np.float32(0.25) and (c['score'] > 0).all()
    assert mr.rescore(c['score'][2:4], c['pred'][2:4], c['label'][2:4]).all()
