"""Every case of tests/sampler_cases.py sits on the edge it is named for - asserted from the NumPy oracle alone, on any machine.  A case
that misses its edge fails HERE instead of silently weakening the GPU comparison in tests/test_rpn_gpu.py / tests/test_targets_gpu.py."""
import numpy as np
import pytest

from oracle import boxes as ob
from tests import sampler_cases as sc

F = np.float32
# what tests/test_rpn_gpu.py::test_proposals_end_to_end_bit_exact already sorts (n_pre clamped to the anchors of its pyramid)
EXISTING_N_PRE = [7677, 600, 3000, 100, 12000, 2048, 2049, 16384]


# ---- A ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_pre', sc.SORT_SHAPES)
def test_sort_shape_has_exactly_n_pre_rows(n_pre):
    c = sc.rpn_sort_shape(n_pre)
    assert c['n_eff'] == n_pre and len(c['want']) == 2
    for w in c['want']:
        assert len(w['pre_nms_index']) == n_pre and w['n_valid'] >= n_pre
        assert 1 <= len(w['rois']) <= c['n_post']


def test_sort_shapes_cover_every_instantiation():
    nps = {sc.sort_np(n) for n in sc.SORT_SHAPES + EXISTING_N_PRE}
    assert {64, 128, 256, 512, 1024, 2048} <= nps                         # k_sort_desc_lds<64> .. <2048>, one workgroup
    assert {p // sc.RUN for p in nps if p > sc.RUN} == {2, 4, 8}             # k_merge_runs<2>, <4>, <8>
    assert {sc.sort_np(n) for n in (4097, 6000, 8192)} == {8192} and sc.sort_np(8193) == 16384 and sc.sort_np(4096) == 4096


@pytest.mark.parametrize('n_pre', [6000, 600])
def test_mixed_batch_valid_counts(n_pre):
    c = sc.rpn_mixed_valid(n_pre)
    v = [w['n_valid'] for w in c['want']]
    assert v[0] > 6000 and 1 <= v[1] <= 2047 and v[2] == 0
    assert len(c['want'][0]['pre_nms_index']) == n_pre and len(c['want'][1]['pre_nms_index']) == min(n_pre, v[1])
    assert len(c['want'][2]['pre_nms_index']) == 0 and len(c['want'][2]['rois']) == 0
    if n_pre == 600:
        assert v[1] < 600                                                      # fewer valid than asked in the single-workgroup sort too


def test_fewer_anchors_than_n_pre():
    c = sc.rpn_fewer_anchors_than_n_pre()
    assert c['anchors'].shape[0] == 75 and c['n_pre'] == 2000 and c['n_eff'] == 75
    assert all(1 <= len(w['pre_nms_index']) <= 75 for w in c['want'])


def test_second_compaction_trip_members_on_both_sides():
    c = sc.rpn_second_compaction_trip()
    A = c['anchors'].shape[0]
    assert A == 524288 + 2048 + 37 and A > sc.COMPACT_TRIP
    pre = c['want'][0]['pre_nms_index']
    assert len(pre) == 300 and (pre < sc.COMPACT_TRIP).sum() >= 100 and (pre >= sc.COMPACT_TRIP).sum() >= 100 and (A - 1) in pre
    assert set(pre) == set(c['planted'])


@pytest.mark.parametrize('n_pre', [600, 6000])
def test_equal_scores_order_is_the_index_alone(n_pre):
    c = sc.rpn_index_only_keys('equal', n_pre)
    for i, w in enumerate(c['want']):
        s = c['scores'][i, :, 1]
        assert np.unique(s).size == 1 and (s[0] > 0) == (i == 0)
        pre = w['pre_nms_index']
        assert len(pre) == n_pre and np.all(np.diff(pre) < 0)
        valid = np.where(sc.rpn_valid(c['locs'][i], c['anchors'], c['img_size'], 16.0))[0]
        np.testing.assert_array_equal(pre, valid[::-1][:n_pre])


@pytest.mark.parametrize('n_pre', [600, 6000])
def test_low_bit_scores_are_three_neighbouring_patterns(n_pre):
    c = sc.rpn_index_only_keys('lowbit', n_pre)
    for i, w in enumerate(c['want']):
        bits = np.unique(c['scores'][i, :, 1].view(np.uint32))
        assert bits.size == 3 and bits.max() - bits.min() == 2
        s = c['scores'][i, w['pre_nms_index'], 1]
        assert len(s) == n_pre and np.unique(s).size >= 2                    # the cut falls behind at least one change of value
        same = np.diff(s) == 0
        assert np.all(np.diff(s) <= 0) and np.all(np.diff(w['pre_nms_index'])[same] < 0)


def test_special_scores_reach_the_sorted_prefix():
    c = sc.rpn_special_scores()
    for i, w in enumerate(c['want']):
        pre, s = w['pre_nms_index'], c['scores'][i, :, 1]
        idx = c['special_index'][i]
        got = s[idx[400:]]
        assert np.isposinf(got[0]) and np.isneginf(got[1]) and got[2] == np.finfo(F).max and got[4] == np.finfo(F).tiny
        assert 0 < got[6] < np.finfo(F).tiny and -np.finfo(F).tiny < got[7] < 0           # denormals of both signs
        z = s[idx[:400]]
        assert np.all(z == 0) and np.signbit(z).sum() == 200 and np.all(np.signbit(z[::2]) != np.signbit(z[1::2]))
        assert len(pre) == 600 and set(idx[:400]) <= set(pre)
        zpos = pre[np.isin(pre, idx[:400])]
        np.testing.assert_array_equal(zpos, np.sort(idx[:400])[::-1])          # +0.0 and -0.0 compare equal: the index decides
        assert np.signbit(s[zpos]).any() and not np.all(np.diff(np.signbit(s[zpos]).astype(int)) <= 0)      # ... not the sign
        assert pre[0] == idx[400] and np.isneginf(s[idx[401]]) and idx[401] not in pre


# ---- B ---------------------------------------------------------------------------------------------------------------
def _counts(lab):
    return int((lab == 1).sum()), int((lab == 0).sum())


def test_anchor_many_positives():
    c = sc.anchor_many_positives()
    p0, _ = _counts(c['label_before'][0])
    p1, _ = _counts(c['label_before'][1])
    assert p0 > 128 and 0 < p1 < 128
    assert _counts(c['label'][0])[0] == 128 and _counts(c['label'][1])[0] == p1
    assert all((c['label'][i] >= 0).sum() == 256 for i in range(2))


def test_anchor_few_negatives():
    c = sc.anchor_few_negatives()
    for i in range(2):
        p, n = _counts(c['label_before'][i])
        assert 0 < p < 128 and 0 < n < 256 - p
        np.testing.assert_array_equal(c['label'][i], c['label_before'][i])      # nothing is disabled
        assert (c['label'][i] >= 0).sum() < 256


@pytest.mark.parametrize('kind', ['zero', 'ones', 'two'])
def test_anchor_equal_keys(kind):
    c = sc.anchor_equal_keys(kind)
    assert np.unique(c['keys']).size == (2 if kind == 'two' else 1)
    for i in range(2):
        p, n = _counts(c['label_before'][i])
        assert p > 128 and n > 128
        if kind != 'two':                                                       # the survivors are the smallest anchor indices
            np.testing.assert_array_equal(np.where(c['label'][i] == 1)[0], np.where(c['label_before'][i] == 1)[0][:128])
            np.testing.assert_array_equal(np.where(c['label'][i] == 0)[0], np.where(c['label_before'][i] == 0)[0][:128])


def test_anchor_empty_beside_objects():
    c = sc.anchor_empty_beside_objects()
    np.testing.assert_array_equal(c['n_gt'], [0, 5, 0])
    inside = sc.anchor_inside(c['anchors'], c['img_size'])
    for i in (0, 2):
        assert _counts(c['label_before'][i]) == (0, len(inside)) and _counts(c['label'][i]) == (0, 256) and not c['loc'][i].any()
    assert _counts(c['label'][1])[0] > 0 and c['loc'][1].any()
    assert not np.array_equal(c['label'][0], c['label'][2])                    # each image by its own keys


def test_anchor_full_gt_cap():
    c = sc.anchor_full_gt_cap()
    assert c['gt'].shape[1] == 256 and list(c['n_gt']) == [256, 255, 1]
    assert np.unique(c['gt'][0], axis=0).shape[0] == 256
    inside, a, argmax, _, _ = sc.ot.AnchorTargetCreator().labels_before_sampling(c['gt'][0], c['anchors'], c['img_size'])
    assert argmax.max() == 255                                                 # the last row of the full table is somebody's best box


def test_anchor_ties():
    c = sc.anchor_ties()
    gt = c['gt'][0, :5]
    inside, a, argmax, max_ious, lab = sc.ot.AnchorTargetCreator().labels_before_sampling(gt, c['anchors'], c['img_size'])
    ious = ob.bbox_iou(a, gt)
    np.testing.assert_array_equal(gt[0], gt[1])
    assert (argmax == 0).any() and not (argmax == 1).any()                    # identical boxes: argmax is the first
    e, m = np.where(inside == c['equal_anchor'])[0][0], np.where(inside == c['mirror_anchor'])[0][0]
    assert ious[e, 2] == 1.0 and argmax[e] == 2
    assert ious[m, 3] == ious[m, 4] == max_ious[m] > 0.3 and argmax[m] == 3     # equal IoU to two different boxes: the first


def test_anchor_zero_area_gt_makes_every_inside_anchor_positive():
    c = sc.anchor_zero_area_gt()
    inside = sc.anchor_inside(c['anchors'], c['img_size'])
    for i in range(2):
        assert _counts(c['label_before'][i]) == (len(inside), 0) and len(inside) > 128
        assert _counts(c['label'][i]) == (128, 0)


def test_anchor_border_touch():
    c = sc.anchor_border_touch()
    A = c['anchors'].shape[0]
    assert A % 64 != 0 and c['anchors'][-1, 2] == c['img_size'][0]
    assert A - 1 in sc.anchor_inside(c['anchors'], c['img_size']) and c['label_before'][0, -1] == 1 and c['loc'][0, -1].any()


# ---- C ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('total', sc.PT_COUNTS)
def test_pt_candidate_counts(total):
    c = sc.pt_candidate_count(total)
    assert np.all(c['n_r'] + c['n_gt'] == total) and c['roi_cap'] + c['gt_cap'] <= 4096
    if total >= 4095:
        assert (c['roi_cap'], c['gt_cap']) == (3840, 256) and np.all(c['n_gt'] == total - 3840) and np.all(c['n_r'] == 3840)
    for w in c['want']:
        assert len(w['max_iou']) == total
        if total == 4096:
            assert w['n_cand'][0] >= 64 and w['n_pos'] == 64 and len(w['keep']) == 256


def test_pt_no_proposals():
    c = sc.pt_no_proposals()
    assert not c['n_r'].any()
    for i, w in enumerate(c['want']):
        assert w['n_cand'] == (c['n_gt'][i], 0) and w['n_pos'] == c['n_gt'][i] == len(w['keep'])


def test_pt_empty_image_of_two():
    c = sc.pt_empty_image_of_two()
    assert list(c['n_gt']) == [4, 0]
    w = c['want'][1]
    assert w['n_pos'] == 0 and w['n_cand'] == (0, c['n_r'][1]) and len(w['keep']) == 256
    assert np.all(w['assign'] == -1) and not w['loc'].any() and not w['label'].any()
    assert c['want'][0]['n_pos'] > 0


def test_pt_short_sets():
    w = sc.pt_short_sets()['want']
    assert 0 < w[0]['n_cand'][0] < 64 and w[0]['n_cand'][1] >= 256 - w[0]['n_cand'][0] and len(w[0]['keep']) == 256
    assert w[1]['n_cand'][0] > 64 and 0 < w[1]['n_cand'][1] < 192 and len(w[1]['keep']) == 64 + w[1]['n_cand'][1] < 256
    assert w[2]['n_cand'][0] > 64 and w[2]['n_cand'][1] == 0 and len(w[2]['keep']) == 64


@pytest.mark.parametrize('kind', ['zero', 'ones', 'class'])
def test_pt_equal_keys(kind):
    c = sc.pt_equal_keys(kind)
    for i, w in enumerate(c['want']):
        assert w['n_cand'][0] > 64 and w['n_cand'][1] > 192                    # more candidates than kept in both classes
        fg = np.where(w['max_iou'] >= F(0.5))[0]
        bg = np.where(w['max_iou'] < F(0.5))[0]
        np.testing.assert_array_equal(w['keep'], np.concatenate([fg[:64], bg[:192]]))       # the smallest candidate indices
        kk = np.concatenate([c['keys'][i, :c['n_r'][i]], c['keys'][i, c['roi_cap']:c['roi_cap'] + c['n_gt'][i]]])
        assert np.unique(kk[fg]).size == 1 and np.unique(kk[bg]).size == 1 and (np.unique(kk).size == 2) == (kind == 'class')


@pytest.mark.parametrize('neg_lo', [0.0, 0.1])
def test_pt_exact_thresholds(neg_lo):
    c = sc.pt_exact_thresholds(neg_lo)
    for w in c['want']:
        assert w['max_iou'][0] == F(0.5) and w['max_iou'][1] == 0
        n_pos = w['n_pos']
        assert 0 in w['keep'][:n_pos] and 0 not in w['keep'][n_pos:]           # IoU 0.5: foreground, not background
        assert (1 in w['keep'][n_pos:]) == (neg_lo == 0.0) and 1 not in w['keep'][:n_pos]
        assert len(w['keep']) < 256                                            # every candidate is taken: membership is the set


@pytest.mark.parametrize('leading', [False, True])
def test_pt_degenerate_gt_nan_is_in_neither_set(leading):
    c = sc.pt_degenerate_gt(leading)
    G = 4 if leading else 3
    w = c['want'][0]
    nr = c['n_r'][0]
    nan = np.where(np.isnan(w['max_iou']))[0]
    zero_area = [nr + g for g in range(G) if c['gt'][0, g, 2] == c['gt'][0, g, 0]] + [30]
    assert sorted(nan) == sorted(zero_area) and len(nan) == (4 if leading else 3)
    assert not set(nan) & set(w['keep']) and w['n_cand'][0] + w['n_cand'][1] == nr + G - len(nan)
    assert len(w['keep']) == w['n_cand'][0] + w['n_cand'][1]                     # everything that is a candidate is kept: the sets are pinned
    if not leading:                                                            # the example of the issue
        np.testing.assert_array_equal(np.isnan(w['max_iou'][nr:]), [False, True, True])


# ---- D ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_pos', sc.MK_N_POS)
def test_mask_keypoint_batch(n_pos):
    c = sc.mask_keypoint_batch(n_pos)
    assert (sc.MK_N, sc.MK_SAMPLE, sc.MK_POS_CAP, sc.MK_GT_CAP) == (2, 256, 64, 6)
    assert not np.array_equal(c['masks'][0], c['masks'][1]) and not np.array_equal(c['kps'][0], c['kps'][1])
    assert not np.array_equal(c['gt_assign'][:64], c['gt_assign'][256:320])
    used = np.zeros(2 * 64, bool)
    for i in range(2):
        used[i * 64:i * 64 + n_pos[i]] = True
    assert np.all(c['want_mask'][~used] == -1) and np.all(c['want_kp'][~used] == -1) and np.all(c['want_mask'][used] >= 0)
    assert len(c['empty_rows']) == sum(n > 1 for n in n_pos)
    for row in c['empty_rows']:
        b = c['sample_roi'][row]
        assert int(b[2]) == int(b[0]) and not c['want_mask'][(row // 256) * 64 + row % 256].any()
    live = c['want_mask'][used]
    assert live.max() == 1 and (c['want_kp'][used] >= 0).any()
    if n_pos[1]:                                                                # the second image's rows come from ITS masks and rows
        assert c['want_mask'][64:64 + n_pos[1]].any()
