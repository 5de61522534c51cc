"""GPU tests of Soft-NMS, box voting and the detection cap (csrc/boxpost.hip, MaskRCNN.use_soft_nms / use_box_voting / use_max_detections;
DESIGN.md section 3.16): the 'hard' method against the hard NMS kernels, 'linear' bit for bit and 'gaussian' within a derived tolerance
against the NumPy restatement (tests/boxpost_reference.py), box voting against its float64 weighted mean with exact vote sets, and the
three switches end to end on the reduced networks of test_predict_gpu.py and test_keypoint_predict_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import boxpost_reference as ref  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from test_tta_gpu import _case, _union_case  # noqa: E402

DEV = 'cuda:0'
F = np.float32
U = 2.0 ** -24                  # unit roundoff of float32
FRAME = 400.0                   # the generators' frame
THRESH = 0.25                   # score threshold of the kernel tests (test_tta_gpu.py's)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dense_case(seed, R, n_class, thresh, quantised=True):
    """Heavily overlapping boxes: R // 16 cluster centres in the 400 x 400 frame, the boxes of a cluster jittered by 10 % of the cluster's
    size around its centre and their sizes by exp(N(0, 0.15^2)); 10 % duplicate boxes; scores k/64 with some exactly at the threshold
    (quantised) or uniform float32."""
    rs = np.random.RandomState(seed)
    n_c = max(R // 16, 1)
    centre, size = rs.uniform(0, FRAME, (n_c, 2)), np.exp(rs.uniform(np.log(20), np.log(120), (n_c, 2)))
    which = rs.randint(0, n_c, R)
    c = centre[which] + rs.standard_normal((R, 2)) * 0.1 * size[which]
    hw = size[which] * np.exp(rs.standard_normal((R, 2)) * 0.15)
    box = np.concatenate([c - hw / 2, c + hw / 2], 1).astype(F)
    dup = rs.rand(R) < 0.1
    box[dup] = box[rs.randint(0, R, int(dup.sum()))]
    prob = rs.rand(R, n_class).astype(F)
    if quantised:
        prob = (np.round(prob * 64) / 64).astype(F)
        prob[rs.rand(R, n_class) < 0.05] = F(thresh)
    return box, prob


GENERATORS = {'sparse': _union_case, 'dense': _dense_case}


def _lists(keep_idx, keep_cnt, keep_score=None):
    cnt = keep_cnt.cpu().numpy()
    idx = keep_idx.cpu().numpy()
    sc = keep_score.cpu().numpy() if keep_score is not None else None
    return cnt, [idx[l, :cnt[l]] for l in range(len(cnt))], None if sc is None else [sc[l, :cnt[l]] for l in range(len(cnt))]


# ---- Soft-NMS: the hard method is the hard NMS ------------------------------------------------------------------------------------------
def test_hard_is_class_nms():
    rois, box = _case(1, 300)
    cb, pb = ops.detect_decode(rois, box, 81, 88, 1.25, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), (480, 500))
    p = pb.cpu().numpy()
    for thresh in (0.05, 0.3):
        cnt, idx, _ = _lists(*ops.class_nms(cb, pb, 1, 80, thresh, 0.3))
        keep_idx, keep_score, keep_cnt = ops.class_soft_nms(cb, pb, 1, 80, thresh, 'hard', 0.3, 0.5)
        cnt2, idx2, sc2 = _lists(keep_idx, keep_cnt, keep_score)
        np.testing.assert_array_equal(cnt, cnt2)
        for l in range(81):
            np.testing.assert_array_equal(idx[l], idx2[l])
            np.testing.assert_array_equal(sc2[l].view(np.int32), p[idx[l], l].view(np.int32))
        assert cnt.sum() > 0 and cnt[0] == 0 and cnt[80] == 0


@pytest.mark.parametrize('R', [513, 1200])
def test_hard_is_class_nms_ws(R):
    n_class = 12
    box, prob = _union_case(R, R, n_class, THRESH)
    cb, pb = _t(box), _t(prob)
    for le in (n_class - 1, n_class):
        cnt, idx, _ = _lists(*ops.class_nms_ws(cb, pb, 1, le, THRESH, 0.3))
        keep_idx, keep_score, keep_cnt = ops.class_soft_nms(cb, pb, 1, le, THRESH, 'hard', 0.3, 0.5)
        cnt2, idx2, sc2 = _lists(keep_idx, keep_cnt, keep_score)
        np.testing.assert_array_equal(cnt, cnt2)
        for l in range(n_class):
            np.testing.assert_array_equal(idx[l], idx2[l])
            np.testing.assert_array_equal(sc2[l].view(np.int32), prob[idx[l], l].view(np.int32))
        assert cnt.sum() > 100


# ---- Soft-NMS: linear, bit for bit ------------------------------------------------------------------------------------------------------
def _linear_inputs(gen, R):
    n_class = 3 if R == 4096 else 12
    box, prob = GENERATORS[gen](R + 7, R, n_class, THRESH)
    if R == 4096:
        prob[:, 2] = prob[:, 2] * F(0.5)            # class 1: about 3000 candidates (the workspace); class 2: under 2048 (LDS)
    elif R > 1:
        prob[:, 5] = np.minimum(prob[:, 5], F(THRESH))          # a class without a candidate
    return n_class, box, prob


@pytest.mark.parametrize('R', [1, 65, 300, 513, 1200, 4096])
@pytest.mark.parametrize('gen', ['sparse', 'dense'])
def test_linear_equals_the_reference_bit_for_bit(gen, R):
    n_class, box, prob = _linear_inputs(gen, R)
    if R == 1:
        prob[0, 1:] = [F(0.5), F(THRESH)] + [F(0.75)] * (n_class - 3)
    rows, scores, k, _ = ref.class_soft_nms(box, prob, 1, n_class, THRESH, 'linear', 0.3, 0.5)
    cb, pb = _t(box), _t(prob)
    for le in (n_class - 1, n_class):
        keep_idx, keep_score, keep_cnt = ops.class_soft_nms(cb, pb, 1, le, THRESH, 'linear', 0.3, 0.5)
        assert keep_idx.shape == (n_class, R) and keep_score.shape == (n_class, R) and keep_cnt.shape == (n_class,)
        cnt, idx, sc = _lists(keep_idx, keep_cnt, keep_score)
        for l in range(n_class):
            if not 1 <= l < le:
                assert cnt[l] == 0
                continue
            assert cnt[l] == len(rows[l]), (l, cnt[l], len(rows[l]))
            np.testing.assert_array_equal(idx[l], rows[l])
            np.testing.assert_array_equal(sc[l].view(np.int32), scores[l].view(np.int32))
            assert (np.diff(sc[l]) <= 0).all() and (sc[l] > F(THRESH)).all()
    if R == 4096:
        n1, n2 = int((prob[:, 1] > F(THRESH)).sum()), int((prob[:, 2] > F(THRESH)).sum())
        assert n1 > 2048 >= n2 > 0, (n1, n2)
    if R > 1:
        assert k >= 1 and sum(len(r) for r in rows.values()) > 0
        if n_class == 12:
            assert len(rows[5]) == 0
    if R >= 300 and gen == 'dense':                 # it decays: linear keeps more than hard does
        hard = ref.class_soft_nms(box, prob, 1, n_class, THRESH, 'hard', 0.3, 0.5)[0]
        assert sum(len(r) for r in rows.values()) > 1.2 * sum(len(r) for r in hard.values())


# ---- Soft-NMS: gaussian, within the derived tolerance -----------------------------------------------------------------------------------
# seeds for which the reference's own smallest gap exceeds 8 * rtol (asserted below), found by running the reference on the CPU
GAUSSIAN_SEEDS = {64: 1, 300: 4}


@pytest.mark.parametrize('R', [64, 300])
def test_gaussian_equals_the_reference_within_the_derived_tolerance(R):
    """The device's expf and NumPy's float32 exp may differ in the last bits.  A score that received k non-unit decays carries at most k
    exponentials and k products that may each differ by one ulp between the two: rtol = 4 * k * 2^-24 allows two ulps per decay.  The
    selection is a function of comparisons between scores and with the threshold; where every such comparison of the reference has a
    relative gap above 8 * rtol, no comparison can come out differently on the device, and the keep lists must be equal."""
    n_class = 4
    box, prob = _dense_case(GAUSSIAN_SEEDS[R], R, n_class, 0.05, quantised=False)
    rows, scores, k, gap = ref.class_soft_nms(box, prob, 1, n_class, 0.05, 'gaussian', 0.3, 0.5)
    rtol = 4 * k * U
    print('gaussian R=%d: k=%d rtol=%.3g gap=%.3g' % (R, k, rtol, gap))
    assert k >= 2 and gap > 8 * rtol, (k, gap, rtol)
    keep_idx, keep_score, keep_cnt = ops.class_soft_nms(_t(box), _t(prob), 1, n_class, 0.05, 'gaussian', 0.3, 0.5)
    cnt, idx, sc = _lists(keep_idx, keep_cnt, keep_score)
    worst = 0.0
    for l in range(1, n_class):
        assert cnt[l] == len(rows[l])
        np.testing.assert_array_equal(idx[l], rows[l])
        worst = max(worst, float(np.max(np.abs(sc[l].astype(np.float64) - scores[l]) / scores[l])))
    print('gaussian R=%d: largest relative score difference %.3g' % (R, worst))
    for l in range(1, n_class):
        np.testing.assert_allclose(sc[l], scores[l], rtol=rtol, atol=0)
    assert cnt[0] == 0 and cnt[1:].sum() > R // 4


# ---- box voting -----------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.0


def _vote_and_check(box, prob, n_class, le, vote_thresh, keep_idx, keep_cnt, exact=None):
    """box_vote against the reference for the given keep lists; returns the reference's set sizes.  exact: None = the float64 mean within
    the summation bound; 'rational' = bit for bit the correctly rounded quotient (inputs whose sums are exact in float32)."""
    cb, pb = _t(box), _t(prob)
    R = box.shape[0]
    out = torch.full((n_class, R, 4), SENTINEL, dtype=torch.float32, device=DEV)
    got_t = ops.box_vote(cb, pb, 1, le, THRESH, vote_thresh, keep_idx, keep_cnt, out=out)
    assert got_t is out
    again = ops.box_vote(cb, pb, 1, le, THRESH, vote_thresh, keep_idx, keep_cnt)
    cnt, idx, _ = _lists(keep_idx, keep_cnt)
    got, got2 = got_t.cpu().numpy(), again.cpu().numpy()
    sizes = []
    for l in range(n_class):
        assert (got[l, cnt[l]:] == F(SENTINEL)).all()             # rows past keep_cnt, and the classes outside the range, are untouched
        if not 1 <= l < le:
            assert cnt[l] == 0
            continue
        np.testing.assert_array_equal(got[l, :cnt[l]].view(np.int32), got2[l, :cnt[l]].view(np.int32))     # the same bits on every run
        want, sz = ref.vote_class(box, prob[:, l], THRESH, vote_thresh, idx[l])
        sizes.append(sz)
        if exact == 'rational':
            np.testing.assert_array_equal(got[l, :cnt[l]].view(np.int32), want.astype(F).view(np.int32))
        else:
            n_l = int((prob[:, l] > F(THRESH)).sum())
            np.testing.assert_allclose(got[l, :cnt[l]], want, rtol=0, atol=(n_l + 2) * U * FRAME)
    return np.concatenate(sizes)


def _keep_lists_of(source, cb, pb, le):
    if source == 'nms':
        return ops.class_nms_ws(cb, pb, 1, le, THRESH, 0.3)
    keep_idx, _, keep_cnt = ops.class_soft_nms(cb, pb, 1, le, THRESH, 'linear', 0.3, 0.5)
    return keep_idx, keep_cnt


@pytest.mark.parametrize('R', [65, 300, 1200])
@pytest.mark.parametrize('gen', ['sparse', 'dense'])
def test_vote_equals_the_weighted_mean(gen, R):
    n_class = 6
    box, prob = GENERATORS[gen](R + 3, R, n_class, THRESH)
    assert np.abs(box).max() <= 1.25 * FRAME                      # the bound's frame (boxes reach a little over the 400 x 400 frame)
    cb, pb = _t(box), _t(prob)
    for source in ('nms', 'soft'):
        for le in (n_class - 1, n_class):
            keep_idx, keep_cnt = _keep_lists_of(source, cb, pb, le)
            for vote_thresh in (0.5, 0.8):
                sizes = _vote_and_check(box, prob, n_class, le, vote_thresh, keep_idx, keep_cnt)
                assert sizes.min() >= 1 and sizes.max() >= 2, (sizes.min(), sizes.max())


@pytest.mark.parametrize('R', [65, 300, 1200])
@pytest.mark.parametrize('gen', ['sparse', 'dense'])
def test_vote_sets_are_exact(gen, R):
    """Integer box coordinates and scores k/64: every product and every partial sum of the vote is an integer multiple of 1/64 below
    2^24 / 64 (asserted), exact in float32 in any order, so the voted box is the correctly rounded quotient of the exact sums - a function
    of the vote set alone.  One voter too many or too few changes the sums: equal bits mean equal vote sets."""
    n_class = 6
    box, prob = GENERATORS[gen](R + 5, R, n_class, THRESH)
    box = np.round(box).astype(F)
    cb, pb = _t(box), _t(prob)
    k64 = (prob * 64).astype(np.int64)
    assert (k64 == prob * 64).all()
    for vote_thresh in (0.5, 0.8):
        keep_idx, keep_cnt = _keep_lists_of('soft', cb, pb, n_class)
        cnt, idx, _ = _lists(keep_idx, keep_cnt)
        for l in range(1, n_class):                               # the exactness condition, from the reference's vote sets
            cand = np.nonzero(prob[:, l] > F(THRESH))[0]
            for k in idx[l]:
                v = cand[ref.box_iou(box[k], box[cand]) >= F(vote_thresh)]
                assert (k64[v, l][:, None] * np.abs(box[v]).astype(np.int64)).sum(0).max() < 2 ** 24
        sizes = _vote_and_check(box, prob, n_class, n_class, vote_thresh, keep_idx, keep_cnt, exact='rational')
        assert sizes.min() >= 1 and sizes.max() >= 2


def test_vote_of_equal_boxes_is_that_box():
    """Every row takes the box of one of 64 disjoint cells, so the reference's vote set of a kept detection is the candidates of its cell
    (IoU 1 with them, 0 with the others; asserted on the reference's set sizes), all with its own box, and the device's voted box must
    equal that box bit for bit (integer coordinates, scores k/64).  This shows that no box of another cell votes and that equal boxes
    average to themselves; it cannot tell which candidates of the cell voted - test_vote_sets_are_exact shows that."""
    R, n_class = 300, 6
    rs = np.random.RandomState(11)
    cell = rs.randint(0, 64, R)
    cy, cx = (cell // 8) * 50, (cell % 8) * 50
    box = np.stack([cy + 5, cx + 5, cy + 45, cx + 35], 1).astype(F)
    prob = (np.round(rs.rand(R, n_class) * 64) / 64).astype(F)
    cb, pb = _t(box), _t(prob)
    keep_idx, keep_cnt = _keep_lists_of('nms', cb, pb, n_class)
    cnt, idx, _ = _lists(keep_idx, keep_cnt)
    for vote_thresh in (0.5, 0.8, 1.0):
        got = ops.box_vote(cb, pb, 1, n_class, THRESH, vote_thresh, keep_idx, keep_cnt).cpu().numpy()
        for l in range(1, n_class):
            assert 0 < cnt[l] <= 64
            np.testing.assert_array_equal(got[l, :cnt[l]].view(np.int32), box[idx[l]].view(np.int32))
            _, sizes = ref.vote_class(box, prob[:, l], THRESH, vote_thresh, idx[l])
            cand = prob[:, l] > F(THRESH)
            np.testing.assert_array_equal(sizes, [int((cand & (cell == cell[k])).sum()) for k in idx[l]])
            assert sizes.max() >= 3


def test_vote_keeps_a_zero_area_box_and_empty_inputs():
    box = np.array([[0, 0, 10, 10], [0, 0, 10, 12], [5, 5, 5, 9], [5, 5, 5, 9]], F)
    prob = np.array([[0, 0.5], [0, 0.25], [0, 0.75], [0, 0.5]], F)
    cb, pb = _t(box), _t(prob)
    keep_idx, keep_score, keep_cnt = ops.class_soft_nms(cb, pb, 1, 2, 0.05, 'linear', 0.3, 0.5)
    assert keep_idx[1, :int(keep_cnt[1])].tolist() == [2, 3, 0] and keep_score[1, :3].tolist() == [0.75, 0.5, 0.5]      # NaN IoU: no effect
    got = ops.box_vote(cb, pb, 1, 2, 0.05, 0.8, keep_idx, keep_cnt).cpu().numpy()
    np.testing.assert_array_equal(got[1, 0], box[2])
    np.testing.assert_array_equal(got[1, 1], box[3])
    np.testing.assert_allclose(got[1, 2], [0, 0, 10, (0.5 * 10 + 0.25 * 12) / 0.75], rtol=0, atol=4 * U * 12)
    z = ops.class_soft_nms(cb[:0], pb[:0], 1, 2, 0.05, 'linear', 0.3, 0.5)          # R == 0: no launch
    assert z[0].shape == (2, 1) and z[1].shape == (2, 1) and z[2].tolist() == [0, 0]
    assert ops.box_vote(cb[:0], pb[:0], 1, 2, 0.05, 0.8, z[0], z[2]).shape == (2, 1, 4)
    with pytest.raises(Exception, match='4096'):
        ops.class_soft_nms(_t(np.zeros((4097, 4), F)), _t(np.zeros((4097, 2), F)), 1, 2, 0.05, 'linear', 0.3, 0.5)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mask_model():
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=5, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.0125                         # random weights: ~uniform class probabilities (1/81 = 0.0123)
    return m


IMG = torch.from_numpy((np.random.RandomState(0).rand(3, 120, 150) * 255).astype(np.float32))
COMBOS = [(s, v, c) for s in (None, 'linear') for v in (None, 0.8) for c in (None, 20) if (s, v, c) != (None, None, None)]


def _switch(m, soft, vote, cap):
    m.use_soft_nms(soft)
    m.use_box_voting(vote)
    m.use_max_detections(cap)


def _check_detections(m, soft, vote, cap, labels, scores, size):
    """labels / scores / m.last_bboxes of one image against the reference applied to m.last_decoded."""
    cls_bbox, prob = (t.cpu().numpy() for t in m.last_decoded)
    l_end = m.n_class - 1 if m.predict_mask else m.n_class
    rows, lab, score, bbox, n_l = ref.suppress(cls_bbox, prob, l_end, m.score_thresh, m.nms_thresh, soft or 'hard', 0.5, vote, cap)
    got_b = m.last_bboxes[0].cpu().numpy()
    np.testing.assert_array_equal(labels.cpu().numpy(), lab)
    np.testing.assert_array_equal(scores.cpu().numpy().view(np.int32), score.view(np.int32))
    if vote is None:
        np.testing.assert_array_equal(got_b.view(np.int32), cls_bbox[rows].view(np.int32))
    else:
        assert np.all(np.abs(got_b - bbox) <= ((n_l + 2) * U * max(size))[:, None])
        assert np.abs(got_b - cls_bbox[rows]).max() > 0                # voting moved a box
    D = len(lab)
    assert D > 0 and (cap is None or D <= cap) and (scores.cpu().numpy() > F(m.score_thresh)).all()
    return D


@pytest.mark.parametrize('tta', [False, True])
@pytest.mark.parametrize('soft,vote,cap', COMBOS)
def test_predict_with_the_switches(mask_model, soft, vote, cap, tta):
    m = mask_model
    size = tuple(IMG.shape[1:])
    try:
        m.use_test_augmentation([160, 224], hflip=True) if tta else m.use_test_augmentation(None)
        _switch(m, None, None, None)
        _, labels0, _ = m.predict([IMG])
        _switch(m, soft, vote, cap)
        masks, labels, scores = m.predict([IMG])
        D = _check_detections(m, soft, vote, cap, labels[0], scores[0], size)
        if cap is not None:
            assert labels0[0].shape[0] > cap == D                    # the cap was in force
        assert masks[0].shape == (D,) + size and masks[0].dtype == torch.bool
        bbox = m.last_bboxes[0]
        with m._inference_mode():                       # the branch on the returned rows, pasted at the returned boxes
            _, bbox2, label2, _, br, mirrors = m._detect_and_branch(IMG, True)
        assert torch.equal(bbox2.view(torch.int32), bbox.view(torch.int32)) and torch.equal(label2, labels[0])
        if mirrors is None:
            want = ops.mask_paste(br, label2.contiguous(), bbox, size)
        else:
            want = ops.mask_paste_prob(ops.tta_mask_merge(br, mirrors, label2.contiguous()), bbox, size)
        assert torch.equal(masks[0], want.bool())
    finally:
        _switch(m, None, None, None)
        m.use_test_augmentation(None)


def test_predict_keypoints_with_the_switches():
    from test_keypoint_predict_gpu import _keypoint_model
    from chainer_maskrcnn.evaluator import SyntheticKeypointEvalDataset
    m = _keypoint_model()
    img = torch.from_numpy(SyntheticKeypointEvalDataset(1, 120, 150)[0][0])
    size = tuple(img.shape[1:])
    _, labels0, _ = m.predict_keypoints([img])
    cap = max(1, labels0[0].shape[0] // 2)
    _switch(m, 'linear', 0.8, cap)
    kps, labels, scores = m.predict_keypoints([img])
    D = _check_detections(m, 'linear', 0.8, cap, labels[0], scores[0], size)
    assert D == cap < labels0[0].shape[0]
    bbox = m.last_bboxes[0]
    with m._inference_mode():
        _, bbox2, _, _, heat, _ = m._detect_and_branch(img, True)
    assert torch.equal(bbox2.view(torch.int32), bbox.view(torch.int32))
    want = ops.keypoint_decode(heat, bbox, m.head.n_keypoints)
    assert kps[0].shape == (D, m.head.n_keypoints, 4) and torch.equal(kps[0].view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('tta', [False, True])
def test_switches_off_again_give_the_earlier_bits(mask_model, tta):
    m = mask_model
    try:
        m.use_test_augmentation([160, 224], hflip=True) if tta else m.use_test_augmentation(None)
        _switch(m, None, None, None)
        masks0, labels0, scores0 = m.predict([IMG])
        bbox0 = m.last_bboxes[0]
        _switch(m, 'gaussian', 0.8, 20)
        _, labels1, scores1 = m.predict([IMG])
        assert labels1[0].shape[0] == 20 and (scores1[0] > m.score_thresh).all()
        _switch(m, None, None, None)
        masks2, labels2, scores2 = m.predict([IMG])
        assert torch.equal(masks0[0], masks2[0]) and torch.equal(labels0[0], labels2[0])
        assert torch.equal(scores0[0].view(torch.int32), scores2[0].view(torch.int32))
        assert torch.equal(bbox0.view(torch.int32), m.last_bboxes[0].view(torch.int32))
    finally:
        _switch(m, None, None, None)
        m.use_test_augmentation(None)
