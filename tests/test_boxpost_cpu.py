"""CPU tests of Soft-NMS, box voting and the detection cap: the NumPy restatement of the rules
(tests/boxpost_reference.py) on hand-computed cases and against oracle.predict.suppress, the cap's order, the validation of
MaskRCNN.use_soft_nms / use_box_voting / use_max_detections, the flag errors of evaluate.py / demo.py / train.py before a model exists,
and the argument errors of the two library entry points without a device."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import boxpost_reference as ref  # noqa: E402
from chainer_maskrcnn import _hip  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from oracle import predict as op  # noqa: E402
from test_tta_gpu import _union_case  # noqa: E402

F = np.float32
BOX = np.array([10, 20, 50, 80], F)


# ---- the rules, by hand --------------------------------------------------------------------------------------------------------------------
def test_iou_is_the_hard_nms_expression():
    b = np.array([[0, 0, 10, 10], [0, 5, 10, 15], [20, 20, 30, 30], [3, 3, 3, 9], [0, 0, 10, 10]], F)
    iou = ref.box_iou(b[0], b)
    assert iou[0] == F(1) and iou[4] == F(1) and iou[2] == F(0)
    assert iou[1] == F(50) / F(150)
    assert iou[3] == F(0)                                         # a zero-area box inside: 0 / 100
    assert np.isnan(ref.box_iou(b[3], b[3:4]))[0]                  # two zero-area boxes: 0 / 0
    for m in ref.METHODS:                                          # NaN: no effect
        assert ref.weight(m, np.array([np.nan], F), 0.3, 0.5)[0] == F(1)


def test_three_identical_boxes_linear_keeps_one():
    box = np.stack([BOX] * 3)
    p = np.array([0.5, 0.9, 0.7], F)
    rows, scores, k, _ = ref.soft_nms_class(box, p, 0.05, 'linear', 0.3, 0.5)
    assert rows.tolist() == [1] and scores.tolist() == [F(0.9)] and k == 1     # IoU 1: the others go to 0
    rows, scores, _, _ = ref.soft_nms_class(box, p, 0.05, 'hard', 0.3, 0.5)
    assert rows.tolist() == [1] and scores.tolist() == [F(0.9)]


def test_three_identical_boxes_gaussian_decay_by_e_minus_two():
    box = np.stack([BOX] * 3)
    p = np.array([0.9, 0.8, 0.7], F)
    e2 = np.exp(F(-1) / F(0.5)).astype(F)                           # exp(-(1 * 1) / 0.5)
    rows, scores, k, _ = ref.soft_nms_class(box, p, 0.01, 'gaussian', 0.3, 0.5)
    assert rows.tolist() == [0, 1, 2] and k == 2
    assert scores.tolist() == [F(0.9), F(0.8) * e2, F(F(0.7) * e2) * e2]
    assert abs(float(e2) - np.exp(-2.0)) < 1e-8
    rows, scores, k, _ = ref.soft_nms_class(box, p, 0.05, 'gaussian', 0.3, 0.5)        # 0.7 e^-4 = 0.0128: under the threshold
    assert rows.tolist() == [0, 1] and scores.tolist() == [F(0.9), F(0.8) * e2]
    rows, _, _, _ = ref.soft_nms_class(box, p, 0.2, 'gaussian', 0.3, 0.5)              # 0.8 e^-2 = 0.108
    assert rows.tolist() == [0]


def test_scores_at_the_threshold():
    box = np.array([[0, 0, 10, 10], [100, 100, 110, 110], [0, 5, 10, 15]], F)
    p = np.array([0.25, 0.5, 0.25], F)
    for m in ref.METHODS:                                          # exactly at the threshold: no candidate
        rows, scores, k, _ = ref.soft_nms_class(box, p, 0.25, m, 0.3, 0.5)
        assert rows.tolist() == [1] and scores.tolist() == [F(0.5)] and k == 0
    # a decayed score exactly equal to the threshold is removed: IoU(0, 2) = 50 / 150 rounds so that 1 - iou = 2/3 (+ 1 ulp); scores
    # 0.75 and 0.375 with IoU exactly 0.5 give 0.375 * 0.5 = 0.1875
    box = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], F)
    assert ref.box_iou(box[0], box)[1] == F(0.5)
    p = np.array([0.75, 0.375], F)
    rows, scores, _, gap = ref.soft_nms_class(box, p, 0.1875, 'linear', 0.3, 0.5)
    assert rows.tolist() == [0] and gap == 0.0
    rows, scores, _, _ = ref.soft_nms_class(box, p, np.nextafter(F(0.1875), F(0)), 'linear', 0.3, 0.5)
    assert rows.tolist() == [0, 1] and scores.tolist() == [F(0.75), F(0.1875)]


def test_tie_order_and_non_increasing_scores():
    box = np.array([[0, 0, 10, 10], [100, 0, 110, 10], [200, 0, 210, 10], [0, 2, 10, 12]], F)
    p = np.array([0.5, 0.5, 0.75, 0.5], F)
    rows, scores, _, _ = ref.soft_nms_class(box, p, 0.05, 'linear', 0.3, 0.5)
    assert rows.tolist() == [2, 3, 1, 0]                            # equal scores: index descending; row 0 decayed by row 3
    assert scores[3] == F(0.5) * (F(1) - ref.box_iou(box[3], box[0:1])[0])
    assert (np.diff(scores) <= 0).all() and (scores > F(0.05)).all()


def test_vote_by_hand():
    box = np.array([[0, 0, 10, 10], [0, 0, 10, 12], [0, 0, 10, 40], [5, 5, 5, 9], [0, 0, 10, 10]], F)
    p = np.array([0.5, 0.25, 0.9, 0.8, 0.04], F)                   # row 4 is no candidate
    out, sizes = ref.vote_class(box, p, 0.05, 0.8, [0, 3, 2])
    assert sizes.tolist() == [2, 0, 1]                             # IoU(0, 1) = 100 / 120; the zero-area box votes for nothing
    np.testing.assert_allclose(out[0], [0, 0, 10, (0.5 * 10 + 0.25 * 12) / 0.75], rtol=1e-15)
    np.testing.assert_array_equal(out[1], box[3])                   # ... and keeps its box
    np.testing.assert_array_equal(out[2], box[2])
    out, sizes = ref.vote_class(box, p, 0.05, 0.25, [0])
    assert sizes.tolist() == [3]


@pytest.mark.parametrize('R', [65, 300, 513])
def test_hard_equals_the_oracle(R):
    n_class, thresh = 12, 0.25
    box, prob = _union_case(R, R, n_class, thresh)
    for predict_mask in (True, False):
        le = n_class - 1 if predict_mask else n_class
        rows, lab, score, bbox, _ = ref.suppress(box, prob, le, thresh, 0.3, 'hard')
        want_idx, want_lab = op.suppress(box, prob, n_class, 0.3, thresh, predict_mask=predict_mask)
        np.testing.assert_array_equal(rows, want_idx)
        np.testing.assert_array_equal(lab, want_lab)
        np.testing.assert_array_equal(score.view(np.int32), prob[want_idx, want_lab + 1].view(np.int32))
        np.testing.assert_array_equal(bbox, box[want_idx].astype(np.float64))
        assert len(rows) > 20


def test_cap_order_and_ties():
    s = np.array([0.5, 0.9, 0.5, 0.7, 0.5, 0.9], F)
    assert ref.cap(s, 6).tolist() == [0, 1, 2, 3, 4, 5] and ref.cap(s, None).tolist() == [0, 1, 2, 3, 4, 5]
    assert ref.cap(s, 3).tolist() == [1, 3, 5]
    assert ref.cap(s, 4).tolist() == [0, 1, 3, 5]                  # the tie at 0.5 goes to the earliest row
    assert ref.cap(s, 5).tolist() == [0, 1, 2, 3, 5]
    assert ref.cap(s, 1).tolist() == [1]
    import torch
    for n in range(1, 7):                                          # the product's expression
        top = torch.sort(torch.from_numpy(s), descending=True, stable=True)[1][:n]
        assert torch.sort(top)[0].tolist() == ref.cap(s, n).tolist()


# ---- the model's switches ------------------------------------------------------------------------------------------------------------------
def _bare_model():
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    return MaskRCNN.__new__(MaskRCNN)


def test_use_soft_nms_validation():
    m = _bare_model()
    m.use_soft_nms('linear')
    assert m.soft_nms == ('linear', 0.5)
    m.use_soft_nms('gaussian', sigma=0.25)
    assert m.soft_nms == ('gaussian', 0.25)
    for bad in ('hard', 'Linear', '', 0, True):
        with pytest.raises(ValueError):
            m.use_soft_nms(bad)
    for bad in (0, -1.0, float('nan'), None, '0.5'):
        with pytest.raises(ValueError):
            m.use_soft_nms('gaussian', sigma=bad)
    assert m.soft_nms == ('gaussian', 0.25)                        # a refused call changes nothing
    m.use_soft_nms(None)
    assert m.soft_nms is None


def test_use_box_voting_and_max_detections_validation():
    m = _bare_model()
    m.use_box_voting(0.8)
    assert m.vote_thresh == 0.8
    m.use_box_voting(1)
    assert m.vote_thresh == 1.0
    for bad in (0, 0.0, -0.1, 1.0001, float('nan'), '0.8', True):
        with pytest.raises(ValueError):
            m.use_box_voting(bad)
    m.use_box_voting(None)
    assert m.vote_thresh is None
    m.use_max_detections(100)
    assert m.max_detections == 100
    m.use_max_detections(np.int64(1))
    assert m.max_detections == 1
    for bad in (0, -5, 2.0, 2.5, '3', True):
        with pytest.raises(ValueError):
            m.use_max_detections(bad)
    m.use_max_detections(None)
    assert m.max_detections is None


def test_the_switches_are_off_until_set_on_an_instance():
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    a, b = MaskRCNN.__new__(MaskRCNN), MaskRCNN.__new__(MaskRCNN)
    assert (a.soft_nms, a.vote_thresh, a.max_detections) == (None, None, None)
    a.use_soft_nms('linear')
    a.use_box_voting(0.8)
    a.use_max_detections(100)
    assert (a.soft_nms, a.vote_thresh, a.max_detections) == (('linear', 0.5), 0.8, 100)
    assert (b.soft_nms, b.vote_thresh, b.max_detections) == (None, None, None)         # another model is not touched
    assert (MaskRCNN.soft_nms, MaskRCNN.vote_thresh, MaskRCNN.max_detections) == (None, None, None)


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------
def test_flag_settings():
    import evaluate
    import demo
    import train
    from train import boxpost_settings
    for mod, argv in ((evaluate, []), (demo, ['--synthetic', '1'])):
        a = mod.build_parser().parse_args(argv)
        assert (a.soft_nms, a.soft_nms_sigma, a.box_vote_thresh, a.max_detections) == ('off', None, 0.0, 0)
        assert boxpost_settings(a.soft_nms, a.soft_nms_sigma, a.box_vote_thresh, a.max_detections) is None
        a = mod.build_parser().parse_args(argv + ['--soft-nms', 'gaussian', '--soft-nms-sigma', '0.25', '--box-vote-thresh', '0.8',
                                                  '--max-detections', '100'])
        assert boxpost_settings(a.soft_nms, a.soft_nms_sigma, a.box_vote_thresh, a.max_detections) == {
            'soft_nms': 'gaussian', 'sigma': 0.25, 'vote_thresh': 0.8, 'max_detections': 100}
        a = mod.build_parser().parse_args(argv + ['--soft-nms', 'linear'])
        assert boxpost_settings(a.soft_nms, a.soft_nms_sigma, a.box_vote_thresh, a.max_detections) == {
            'soft_nms': 'linear', 'sigma': 0.5, 'vote_thresh': None, 'max_detections': None}
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(argv + ['--soft-nms', 'hard'])          # the identity method is not offered
    for keypoints in (False, True):
        a = train.build_parser(keypoints=keypoints).parse_args([])
        assert (a.eval_soft_nms, a.eval_soft_nms_sigma, a.eval_box_vote_thresh, a.eval_max_detections) == ('off', None, 0.0, 0)
        a = train.build_parser(keypoints=keypoints).parse_args(['--eval-soft-nms', 'linear', '--eval-max-detections', '50'])
        assert boxpost_settings(a.eval_soft_nms, a.eval_soft_nms_sigma, a.eval_box_vote_thresh, a.eval_max_detections, '--eval-') == {
            'soft_nms': 'linear', 'sigma': 0.5, 'vote_thresh': None, 'max_detections': 50}
    m = _bare_model()
    train.use_boxpost(m, {'soft_nms': 'gaussian', 'sigma': 0.25, 'vote_thresh': 0.8, 'max_detections': 100})
    assert (m.soft_nms, m.vote_thresh, m.max_detections) == (('gaussian', 0.25), 0.8, 100)
    train.use_boxpost(m, None)
    assert (m.soft_nms, m.vote_thresh, m.max_detections) == (('gaussian', 0.25), 0.8, 100)


BAD_FLAGS = [['--soft-nms', 'gaussian', '--soft-nms-sigma', '0'], ['--soft-nms', 'gaussian', '--soft-nms-sigma', '-1'],
             ['--soft-nms', 'linear', '--soft-nms-sigma', '0.5'], ['--soft-nms-sigma', '0.5'], ['--box-vote-thresh', '1.5'],
             ['--box-vote-thresh', '-0.1'], ['--box-vote-thresh', 'nan'], ['--max-detections', '-1']]


@pytest.mark.parametrize('flags', BAD_FLAGS)
def test_flag_errors_come_before_the_model(flags, monkeypatch, tmp_path):
    import evaluate
    import demo
    import train
    from chainer_maskrcnn.model import maskrcnn

    def no_model(*a, **k):
        raise AssertionError('a model was built')
    monkeypatch.setattr(evaluate, 'build_model', no_model)
    monkeypatch.setattr(demo, 'build_model', no_model)
    monkeypatch.setattr(maskrcnn.MaskRCNN, '__init__', no_model)
    with pytest.raises(ValueError, match=flags[-2].lstrip('-').split('-')[0]):
        evaluate.run(evaluate.build_parser().parse_args(['--synthetic', '1', '--out', str(tmp_path)] + flags))
    with pytest.raises(ValueError):
        demo.run(demo.build_parser().parse_args(['--synthetic', '1', '--out', str(tmp_path)] + flags))
    eval_flags = [f.replace('--', '--eval-', 1) if f.startswith('--') else f for f in flags]
    for keypoints in (False, True):
        argv = ['--synthetic', '1', '--eval-interval', '2', '--out', str(tmp_path)] + (['--eval-metric', 'keypoint_coco'] if keypoints else [])
        with pytest.raises(ValueError, match='--eval-'):
            train.run(train.build_parser(keypoints=keypoints).parse_args(argv + eval_flags), keypoints=keypoints)


@pytest.mark.parametrize('flags', [['--eval-soft-nms', 'linear'], ['--eval-box-vote-thresh', '0.8'], ['--eval-max-detections', '100']])
def test_train_refuses_the_flags_without_an_evaluator(flags, monkeypatch, tmp_path):
    import train
    from chainer_maskrcnn.model import maskrcnn

    def no_model(*a, **k):
        raise AssertionError('a model was built')
    monkeypatch.setattr(maskrcnn.MaskRCNN, '__init__', no_model)
    for keypoints in (False, True):
        with pytest.raises(ValueError, match='--eval-interval'):
            train.run(train.build_parser(keypoints=keypoints).parse_args(['--synthetic', '1', '--out', str(tmp_path)] + flags), keypoints=keypoints)


# ---- the library's entry points ------------------------------------------------------------------------------------------------------------
def test_argument_errors_do_not_need_a_device():
    lib = _hip.lib()
    buf = (ctypes.c_char * 4096)()                    # host memory standing in for device buffers: no call below reaches a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def soft(cls_bbox=p, prob=p, R=300, n_class=81, lb=1, le=80, method=1, sigma=0.5, keep_idx=p, keep_score=p, keep_cnt=p, ws=None, nb=0):
        return lib.mrcnn_class_soft_nms_f32(cls_bbox, prob, R, n_class, lb, le, 0.05, method, 0.3, sigma, keep_idx, keep_score, keep_cnt, ws, nb, None)

    def vote(cls_bbox=p, prob=p, R=300, n_class=81, lb=1, le=80, vt=0.8, keep_idx=p, keep_cnt=p, keep_box=p, st=0.05):
        return lib.mrcnn_box_vote_f32(cls_bbox, prob, R, n_class, lb, le, st, vt, keep_idx, keep_cnt, keep_box, None)
    need = lib.mrcnn_class_soft_nms_workspace_bytes(4096, 81)
    assert need == 81 * 4096 * 24 and lib.mrcnn_class_soft_nms_workspace_bytes(2048, 81) == 0
    assert lib.mrcnn_class_soft_nms_workspace_bytes(2049, 3) == 3 * 2049 * 24
    assert lib.mrcnn_class_soft_nms_workspace_bytes(4097, 81) == 0 and lib.mrcnn_class_soft_nms_workspace_bytes(0, 81) == 0
    soft_cases = [(dict(cls_bbox=None), -1, b'cls_bbox'), (dict(prob=None), -1, b'prob'), (dict(keep_idx=None), -1, b'keep_idx'),
                  (dict(keep_score=None), -1, b'keep_score'), (dict(keep_cnt=None), -1, b'keep_cnt'), (dict(R=0), -1, b'R'),
                  (dict(R=-3), -1, b'R'), (dict(R=4097), -2, b'4096'), (dict(n_class=0), -1, b'n_class'), (dict(lb=-1), -1, b'range'),
                  (dict(le=82), -1, b'range'), (dict(lb=5, le=4), -1, b'range'), (dict(method=3), -1, b'method'),
                  (dict(method=-1), -1, b'method'), (dict(sigma=0.0), -1, b'sigma'), (dict(sigma=-0.5), -1, b'sigma'),
                  (dict(sigma=float('nan')), -1, b'sigma'), (dict(R=4096), -3, b'workspace'), (dict(R=2049, ws=p, nb=100), -3, b'workspace'),
                  (dict(R=4096, ws=p + 4, nb=need), -1, b'aligned'), (dict(cls_bbox=p + 4), -1, b'aligned')]
    vote_cases = [(dict(cls_bbox=None), -1, b'cls_bbox'), (dict(prob=None), -1, b'prob'), (dict(keep_idx=None), -1, b'keep_idx'),
                  (dict(keep_cnt=None), -1, b'keep_cnt'), (dict(keep_box=None), -1, b'keep_box'), (dict(R=0), -1, b'R'),
                  (dict(R=4097), -2, b'4096'), (dict(n_class=-1), -1, b'n_class'), (dict(lb=-1), -1, b'range'), (dict(le=82), -1, b'range'),
                  (dict(vt=0.0), -1, b'vote_thresh'), (dict(vt=1.5), -1, b'vote_thresh'), (dict(vt=float('nan')), -1, b'vote_thresh'),
                  (dict(keep_box=p + 4), -1, b'aligned'), (dict(st=-0.01), -1, b'score_thresh'), (dict(st=float('nan')), -1, b'score_thresh')]
    for fn, name, cases in ((soft, b'class_soft_nms', soft_cases), (vote, b'box_vote', vote_cases)):
        for kw, code, word in cases:
            rc = fn(**kw)
            assert rc == code, (name, kw, rc)
            assert name in lib.mrcnn_last_error() and word in lib.mrcnn_last_error(), (kw, lib.mrcnn_last_error())
            with pytest.raises(_hip.MrcnnHipError):
                _hip.check(rc)
    import torch
    with pytest.raises(_hip.MrcnnHipError):                                              # no CPU fallback
        ops.class_soft_nms(torch.zeros(4, 4), torch.zeros(4, 3), 1, 3, 0.05, 'linear', 0.3, 0.5)
    with pytest.raises(_hip.MrcnnHipError):
        ops.box_vote(torch.zeros(4, 4), torch.zeros(4, 3), 1, 3, 0.05, 0.8, torch.zeros((3, 4), dtype=torch.int32),
                     torch.zeros((3,), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.class_soft_nms(torch.zeros(4, 4), torch.zeros(4, 3), 1, 3, 0.05, 'soft', 0.3, 0.5)
    for name, n in (('mrcnn_class_soft_nms_f32', 16), ('mrcnn_box_vote_f32', 12), ('mrcnn_class_soft_nms_workspace_bytes', 2)):
        assert len(_hip.SIGNATURES[name][1]) == n
    assert _hip.SIGNATURES['mrcnn_class_soft_nms_workspace_bytes'][0] is ctypes.c_size_t


def test_header_and_binding_agree_on_the_constants():
    import re
    src = open(_hip.HEADER_PATH).read()
    defs = {k: int(v) for k, v in re.findall(r'#define (MRCNN_(?:SOFT_NMS|BOXPOST)_[A-Z_]+) (\d+)', src)}
    assert defs == {'MRCNN_BOXPOST_MAX': ops.BOXPOST_MAX, 'MRCNN_SOFT_NMS_LDS_MAX': 2048, 'MRCNN_SOFT_NMS_HARD': ops.SOFT_NMS_METHODS['hard'],
                    'MRCNN_SOFT_NMS_LINEAR': ops.SOFT_NMS_METHODS['linear'], 'MRCNN_SOFT_NMS_GAUSSIAN': ops.SOFT_NMS_METHODS['gaussian']}
    assert _hip.lib().mrcnn_abi_version() == _hip.ABI_VERSION == 10
