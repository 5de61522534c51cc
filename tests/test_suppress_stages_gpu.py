"""GPU tests of the one selection path of MaskRCNN (_suppress) on the reduced network of test_predict_gpu.py: with every
optional stage off - never set, set and reset, or a detection cap that does not bind - predict() gives the same bits, and with every stage
on the selection over a 4096-row union (the workspace kernels) is the composition class_soft_nms -> box_vote -> stable top-k."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402
from chainer_maskrcnn.utils.synthetic import make_batch  # noqa: E402
from test_tta_gpu import _eq, _t, _union_case  # noqa: E402

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def model():
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=5, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.0125                         # random weights: ~uniform class probabilities (1/81 = 0.0123)
    return m


def _predict(m, img):
    masks, labels, scores = m.predict([img])
    return masks[0], labels[0], scores[0], m.last_bboxes[0]


def test_stages_off_give_the_same_bits(model):
    m = model
    img = torch.from_numpy(np.ascontiguousarray(make_batch(2000003, 1, 96, 128)['imgs'][0] * 255, np.float32))
    want = _predict(m, img)
    D = int(want[1].shape[0])
    assert D >= 2 and len(torch.unique(want[1])) >= 2 and bool(want[0].any())      # not an equality of empty lists
    try:
        m.use_soft_nms('gaussian', 0.4)
        m.use_box_voting(0.8)
        m.use_max_detections(1)
        m.use_test_augmentation([160, 224], hflip=True)
        assert int(_predict(m, img)[1].shape[0]) == 1                              # they were on
        m.use_soft_nms(None)
        m.use_box_voting(None)
        m.use_max_detections(None)
        m.use_test_augmentation(None)
        for a, b in zip(_predict(m, img), want):                                   # set and reset
            _eq(a, b)
        for n in (D, D + 7):                                                       # a cap that does not bind
            m.use_max_detections(n)
            for a, b in zip(_predict(m, img), want):
                _eq(a, b)
    finally:
        m.use_soft_nms(None)
        m.use_box_voting(None)
        m.use_max_detections(None)
        m.use_test_augmentation(None)


def _composition(m, cls_bbox, prob, levels, view, soft, vote, cap):
    """The rule of _suppress with every stage on, from the public pieces: Soft-NMS keep lists and decayed scores, voted boxes of the kept
    rows, classes concatenated in order, then the ``cap`` highest scores (ties to the earlier row) in their order."""
    l_end = m.n_class - 1
    keep_idx, keep_score, keep_cnt = ops.class_soft_nms(cls_bbox, prob, 1, l_end, m.score_thresh, soft[0], m.nms_thresh, soft[1])
    keep_box = ops.box_vote(cls_bbox, prob, 1, l_end, m.score_thresh, vote, keep_idx, keep_cnt)
    cnt = keep_cnt.cpu().tolist()
    sel, lab, sc, bb = [], [], [], []
    for l in range(1, l_end):
        if cnt[l]:
            sel.append(keep_idx[l, :cnt[l]])
            lab.append(torch.full((cnt[l],), l - 1, dtype=torch.int32, device=prob.device))
            sc.append(keep_score[l, :cnt[l]])
            bb.append(keep_box[l, :cnt[l]])
    sel, lab, score, bbox = torch.cat(sel).long(), torch.cat(lab), torch.cat(sc), torch.cat(bb)
    n_before = int(sel.shape[0])
    if n_before > cap:
        top = torch.sort(score, descending=True, stable=True)[1][:cap]
        top = torch.sort(top)[0]
        sel, lab, score, bbox = sel[top], lab[top], score[top], bbox[top]
    return (bbox, lab, score, levels[sel], view[sel]), n_before


def test_every_stage_on_a_4096_row_union_equals_the_composition(model):
    m = model
    R, thresh = 4096, 0.75                          # ~1000 candidates per class: above the 512 rows of the single-view kernel
    box, prob = _union_case(R, R, m.n_class, thresh)
    rs = np.random.RandomState(7)
    cls_bbox, prob = _t(box), _t(prob)
    levels, view = _t(rs.randint(0, 4, R).astype(np.int32)), _t(rs.randint(0, 8, R).astype(np.int32))
    keep = m.score_thresh
    try:
        m.score_thresh = thresh
        m.use_soft_nms('linear')
        m.use_box_voting(0.8)
        m.use_max_detections(100)
        got = m._suppress(cls_bbox, prob, levels, view=view)
        want, n_before = _composition(m, cls_bbox, prob, levels, view, m.soft_nms, 0.8, 100)
    finally:
        m.score_thresh = keep
        m.use_soft_nms(None)
        m.use_box_voting(None)
        m.use_max_detections(None)
    assert len(got) == 5 and n_before > 100 == int(got[1].shape[0]) and len(torch.unique(got[1])) >= 2
    for a, b in zip(got, want):
        _eq(a, b)
