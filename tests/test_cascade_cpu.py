"""Cascade R-CNN box stages, everything that needs no device: the NumPy restatement of the stage-to-stage rules
(tests/cascade_reference.py) against the oracle and on the cases the GPU test runs, the constructor's checks, the parameter layout, the NPZ
mapping, the flags of the four scripts and the resume record, the ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from chainer_maskrcnn import _hip
from chainer_maskrcnn._hip import ops
from chainer_maskrcnn.model.maskrcnn import CASCADE_STDS, MaskRCNN, cascade_settings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cascade_reference as cr  # noqa: E402
from oracle import boxes as ob  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
IOUS = (0.5, 0.6, 0.7)
CASES = cr.random_cases()


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def test_float32_restatement_is_the_oracles_arithmetic():
    """loc2bbox, bbox_iou, bbox2loc and the level map of the float32 restatement give the bits of oracle/boxes.py."""
    rs = np.random.RandomState(1)
    y1, x1 = rs.uniform(0, 100, 200), rs.uniform(0, 100, 200)
    a = np.stack([y1, x1, y1 + rs.uniform(1, 80, 200), x1 + rs.uniform(1, 80, 200)], 1).astype(np.float32)
    b = a[rs.permutation(200)][:7] + rs.uniform(-3, 3, (7, 4)).astype(np.float32)
    loc = (rs.standard_normal((200, 4)) * 0.3).astype(np.float32)
    np.testing.assert_array_equal(cr.loc2bbox(a, loc, np.float32), ob.loc2bbox(a, loc))
    np.testing.assert_array_equal(cr.bbox_iou(a, b, np.float32), ob.bbox_iou(a, b))
    d = b[rs.randint(0, 7, 200)]
    np.testing.assert_array_equal(cr.bbox2loc(a, d, np.float32), ob.bbox2loc(a, d))
    # the level: NumPy's float32 log2 and the double one the kernel rounds may differ in the last bit, the floor does not on these boxes
    lev = np.clip(np.floor(cr.level_argument(a, np.float32)), 0, 4)
    np.testing.assert_array_equal(lev, ob.map_rois_to_fpn_levels(a))


@pytest.mark.parametrize('name,case,thr,sp,sn,size', CASES, ids=[c[0] for c in CASES])
def test_random_cases_have_no_row_near_a_decision(name, case, thr, sp, sn, size):
    """The float32 and the float64 restatement agree on every label, assignment and level, and NO row's float64 maximum IoU lies within 1e-5
    of the threshold, NO row's best two IoUs are closer than 1e-5, NO row's level argument is within 1e-5 of an integer: the GPU test
    compares the integer outputs on every row and exempts nothing."""
    f64 = cr.run_case(case, thr, sp, sn, size, np.float64, details=True)
    f32 = cr.run_case(case, thr, sp, sn, size, np.float32)
    for k in ('label', 'gt_assign', 'levels'):
        np.testing.assert_array_equal(f64[k], f32[k], err_msg=k)
    mx, second, larg = f64['max_iou'], f64['second_iou'], f64['level_arg']
    with np.errstate(invalid='ignore'):
        near = (np.abs(mx - thr) < 1e-5) | (np.abs(mx - second) < 1e-5) | (np.abs(larg - np.round(larg)) < 1e-5)
    share = float(near.mean())
    assert share == 0.0, (name, np.nonzero(near)[0])
    lab = f64['label']
    assert (lab > 0).any() and (lab == 0).any() and (lab < 0).any()
    pad = case['prev_label'] < 0
    assert pad.any() and not f64['roi'][pad].any() and (lab[pad] == -1).all()
    assert len(np.unique(f64['levels'])) >= 2
    assert np.isfinite(f64['gt_loc']).all() and not f64['gt_loc'][lab <= 0].any()


def test_geometries_are_the_issues():
    assert [g for g, _ in cr.GEOMETRIES] == [(2, 8, 4), (2, 64, 5), (1, 300, 3)] and cr.GEOMETRIES[0][1] == (3, 0)
    assert len(CASES) == 12 and {c[2] for c in CASES} == {0.6, 0.7}
    assert sum(isinstance(c[5], np.ndarray) for c in CASES) == 6


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_edge_cases_by_the_reference(dtype):
    c = cr.edge_case()
    for size in (c['pair'], c['hw']):
        o = cr.refine(c['rois'], c['box_out'], cr.LOC0, c['N'], cr.MEAN, cr.EDGE_STD, size, c['prev_label'], c['gt_boxes'], c['gt_labels'],
                      c['n_gt'], cr.EDGE_THRESH, cr.EDGE_STD, dtype=dtype, details=True)
        for k, v in c['expect'].items():
            np.testing.assert_array_equal(o[k], v, err_msg=k)
        assert o['max_iou'][0] == 0.75                                    # exactly the threshold: foreground
        assert o['label'][0] == 4 and o['gt_assign'][0] == 0              # two equal IoUs: the first
        assert o['label'][1] == -1 and np.isfinite(o['roi']).all()        # clipped to zero area: ignored
        assert (o['roi'][2] == (0, 0, 100, 100)).all()                    # +88: the full extent
        assert np.isfinite(o['gt_loc']).all() and not o['gt_loc'][o['label'] <= 0].any()
        np.testing.assert_allclose(o['gt_loc'][0], [0, 5. / 30, 0, np.log(40. / 30)], rtol=1e-6)
        infer = cr.refine(c['rois'], c['box_out'], cr.LOC0, c['N'], cr.MEAN, cr.EDGE_STD, size, c['prev_label'], dtype=dtype)
        assert sorted(infer) == ['levels', 'roi', 'rois_xy5']
        for k in infer:
            np.testing.assert_array_equal(infer[k], o[k])


def test_nan_handling_of_the_reference_follows_numpy():
    """Two zero-area boxes give a NaN IoU: the NaN wins the maximum, the first NaN stays, and a NaN maximum is background."""
    rois = np.array([[10, 10, 10.5, 20]], np.float32)
    box_out = np.zeros((1, cr.LD), np.float32)
    gt = np.array([[[0, 0, 50, 50], [30, 30, 30, 30], [40, 40, 40, 40]]], np.float32)
    # a degenerate but non-empty refined box cannot give 0/0; the rule is exercised on the IoU matrix itself
    iou = cr.bbox_iou(np.array([[5, 5, 5, 5]], np.float32), gt[0], np.float32)
    assert np.isnan(iou[0, 1]) and np.isnan(iou[0, 2]) and iou.argmax(axis=1)[0] == 1 and np.isnan(iou.max(axis=1)[0])
    o = cr.refine(rois, box_out, cr.LOC0, 1, cr.MEAN, cr.EDGE_STD, (100., 100.), None, gt, np.array([[1, 2, 3]], np.int32), [3], 0.5, cr.EDGE_STD)
    assert o['label'][0] == 0 and o['gt_assign'][0] == 0


def test_prob_mean_is_the_stage_order_mean():
    rs = np.random.RandomState(2)
    outs = [rs.standard_normal((5, cr.LD)).astype(np.float32) for _ in range(3)]
    outs[1][2, 0] = 1e4
    p = cr.prob_mean(outs, 81)
    sm = [torch.softmax(torch.from_numpy(o[:, :81]).double(), 1).numpy() for o in outs]
    np.testing.assert_allclose(p, (sm[0] + sm[1] + sm[2]) / 3, rtol=1e-12, atol=1e-300)
    assert np.isfinite(p).all() and np.abs(p.sum(1) - 1).max() < 1e-12


# ---- the constructor ----------------------------------------------------------------------------------------------------------------------
def _model(seed=1, keypoints=False, **kw):
    if keypoints:
        return MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', device='cpu', seed=seed, _test_shrink=SHRINK, **kw)
    return MaskRCNN(n_fg_class=5, device='cpu', seed=seed, _test_shrink=SHRINK, **kw)


def test_cascade_settings_and_their_refusals():
    assert cascade_settings(None) is None
    assert cascade_settings(IOUS) == (IOUS, CASCADE_STDS)
    assert cascade_settings((0.5, 0.6)) == ((0.5, 0.6), CASCADE_STDS[:2])
    four = cascade_settings((0.5, 0.6, 0.7, 0.8))[1]
    assert four[0] == CASCADE_STDS[0] and four[3] == (0.025, 0.025, 0.05, 0.05) and four[1] == (0.05, 0.05, 0.1, 0.1)
    own = ((0.07, 0.07, 0.14, 0.14), (0.04, 0.04, 0.08, 0.08))
    assert cascade_settings(IOUS, own)[1] == (CASCADE_STDS[0],) + own
    assert cascade_settings(IOUS, (CASCADE_STDS[0],) + own)[1] == (CASCADE_STDS[0],) + own
    for bad in ((0.5,), (0.5, 0.6, 0.7, 0.8, 0.9), (0.5, 0.7, 0.6), (0.6, 0.7), (0.5, 1.0), 'abc'):
        with pytest.raises(ValueError, match='cascade_ious'):
            cascade_settings(bad)
    with pytest.raises(ValueError, match='cascade_stds'):
        cascade_settings(IOUS, (own[0],))
    with pytest.raises(ValueError, match='cascade_stds'):
        cascade_settings(IOUS, ((0.1, 0.1, 0.2), (0.1, 0.1, 0.2, 0.2)))
    with pytest.raises(ValueError, match='cascade_stds'):
        cascade_settings(IOUS, ((0.1, 0.1, 0.0, 0.2), (0.1, 0.1, 0.2, 0.2)))
    with pytest.raises(ValueError, match='cascade_stds'):
        cascade_settings(None, own)


def test_model_refuses_bad_cascades_and_the_legacy_heads():
    for bad in ((0.5,), (0.5, 0.7, 0.6), (0.5, 0.6, 0.7, 0.8, 0.9)):
        with pytest.raises(ValueError, match='cascade_ious'):
            _model(cascade_ious=bad)
    for arch, backbone in (('res5', 'c4'), ('light', 'fpn')):
        with pytest.raises(ValueError, match='cascade_ious'):
            MaskRCNN(n_fg_class=5, backbone=backbone, head_arch=arch, device='cpu', _test_shrink=dict(width_div=4) if arch == 'res5' else SHRINK,
                     cascade_ious=IOUS)
    m = _model(cascade_ious=IOUS)
    with pytest.raises(ValueError, match='cascade'):
        m.use_test_augmentation([600, 800])
    m.use_test_augmentation(None)
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain
    chain = FPNMaskRCNNTrainChain(m)
    assert chain.proposal_target_creator.pos_iou_thresh == 0.5


def test_loss_rows_are_the_written_out_table():
    """The rows of the step's losses tensor and the observation keys, for 0 .. 3 later box stages with and without the MaskIoU and the
    point head: the reference's five, the stages' (loc, cls) pairs, maskiou_loss, point_loss."""
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, loss_rows
    five = [('rpn_loc_loss', 0), ('rpn_cls_loss', 1), ('roi_loc_loss', 2), ('roi_cls_loss', 3), ('mask_loss', 4)]
    s2, s3, s4 = ([('roi_loc_loss_s%d' % k, r), ('roi_cls_loss_s%d' % k, r + 1)] for k, r in ((2, 5), (3, 7), (4, 9)))
    table = {(0, False, False): (five, 5),
             (0, True, False): (five + [('maskiou_loss', 5)], 6),
             (0, False, True): (five + [('point_loss', 5)], 6),
             (0, True, True): (five + [('maskiou_loss', 5), ('point_loss', 6)], 7),
             (1, False, False): (five + s2, 7),
             (1, True, False): (five + s2 + [('maskiou_loss', 7)], 8),
             (1, False, True): (five + s2 + [('point_loss', 7)], 8),
             (1, True, True): (five + s2 + [('maskiou_loss', 7), ('point_loss', 8)], 9),
             (2, False, False): (five + s2 + s3, 9),
             (2, True, False): (five + s2 + s3 + [('maskiou_loss', 9)], 10),
             (2, False, True): (five + s2 + s3 + [('point_loss', 9)], 10),
             (2, True, True): (five + s2 + s3 + [('maskiou_loss', 9), ('point_loss', 10)], 11),
             (3, False, False): (five + s2 + s3 + s4, 11),
             (3, True, False): (five + s2 + s3 + s4 + [('maskiou_loss', 11)], 12),
             (3, False, True): (five + s2 + s3 + s4 + [('point_loss', 11)], 12),
             (3, True, True): (five + s2 + s3 + s4 + [('maskiou_loss', 11), ('point_loss', 12)], 13)}
    for (later, mask_iou, point), want in table.items():
        assert loss_rows(later, mask_iou, point) == want, (later, mask_iou, point)
    assert loss_rows(0) == (five, 5)
    chain = FPNMaskRCNNTrainChain(_model(cascade_ious=IOUS, mask_iou=True))        # the chain sizes its losses tensor from the model's heads
    assert (chain._loss_rows, chain._n_loss_rows) == table[(2, True, False)]


@pytest.mark.parametrize('keypoints', [False, True], ids=['mask', 'keypoint'])
def test_cascade_adds_only_its_own_parameters_behind_the_head(keypoints):
    plain, none = _model(keypoints=keypoints), _model(keypoints=keypoints, cascade_ious=None)
    assert plain.ps.offsets == none.ps.offsets and list(plain.ps.offsets) == list(none.ps.offsets) and torch.equal(plain.ps.params, none.ps.params)
    assert plain.cascade is None and not plain.cascade_heads and plain.box_stages == [plain.head] and plain.head.pool_grad_scale is None
    K = 2 if keypoints else 3
    m = _model(keypoints=keypoints, cascade_ious=IOUS[:K])
    added = [n for n in m.ps.offsets if n not in plain.ps.offsets]
    per_stage = ['conv1/W', 'conv1/b', 'fc1/W', 'fc1/b', 'fc2/W', 'fc2/b', 'score_cls_loc/W', 'score_cls_loc/b']
    assert added == ['head/cascade%d/%s' % (k, s) for k in range(2, K + 1) for s in per_stage]
    assert list(m.ps.offsets)[:len(plain.ps.offsets)] == list(plain.ps.offsets)        # registered behind everything else
    for n in plain.ps.offsets:          # every extractor / RPN / stage-1 name keeps its offset, shape and initial value
        assert m.ps.offsets[n] == plain.ps.offsets[n], n
        assert torch.equal(m.ps.p(n), plain.ps.p(n)), n
    last_head = max(o + int(np.prod(s)) for n, (o, s) in plain.ps.offsets.items() if n.startswith('head/'))
    assert all(m.ps.offsets[n][0] >= last_head for n in added)
    for k, st in enumerate(m.cascade_heads, 2):
        assert not hasattr(st, 'mask_convs') and not hasattr(st, 'deconv1')
        for s in per_stage:
            assert m.ps.offsets['head/cascade%d/%s' % (k, s)][1] == m.ps.offsets['head/' + s][1]
        assert float(m.ps.p('head/cascade%d/fc1/W' % k).abs().max()) > 0
        assert not torch.equal(m.ps.p('head/cascade%d/fc1/W' % k), m.ps.p('head/fc1/W'))
    assert m.cascade_stds == CASCADE_STDS[:K]
    inv = np.float32(1.0) / np.float32(K)
    assert all(h.pool_grad_scale is m.head.pool_grad_scale and float(h.pool_grad_scale[0]) == float(inv) for h in m.box_stages)
    gn = _model(keypoints=keypoints, cascade_ious=IOUS[:K], head_norm='gn', gn_groups=16)
    assert all(st.gn1 is not None and st.gn1.groups == 16 and st.conv1.relu is False for st in gn.cascade_heads)
    assert 'head/cascade2/conv1/gn/gamma' in gn.ps.offsets


def test_npz_round_trip_of_a_cascade_model(tmp_path):
    from chainer_maskrcnn.utils.chainer_npz import ChainerNpzMap, load_npz, save_npz
    a, b = _model(1, cascade_ious=IOUS, head_norm='gn', gn_groups=16), _model(2, cascade_ious=IOUS, head_norm='gn', gn_groups=16)
    for n in a.ps.offsets:
        if n.startswith('head/cascade') and n.endswith('/b'):
            v = a.ps.p(n)
            v[:3] = torch.tensor([0.5, -1.0, 2.0])
    d = ChainerNpzMap(a).to_chainer()
    h = a.head
    for k in (2, 3):            # Chainer link paths and layouts like the stage-1 head's
        pre = 'head/cascade%d/' % k
        assert d[pre + 'score/W'].shape == d['head/score/W'].shape == (h.n_class, h.fc2.cout)
        assert d[pre + 'cls_loc/W'].shape == (4, h.fc2.cout) and d[pre + 'cls_loc/b'].shape == (4,)
        assert d[pre + 'fc1/W'].shape == d['head/fc1/W'].shape and d[pre + 'fc2/W'].shape == d['head/fc2/W'].shape
        assert d[pre + 'conv1/W'].shape == d['head/conv1/W'].shape and d[pre + 'conv1/gn/gamma'].shape == (h.channels,)
        assert not any(key.startswith(pre + 'mask') or key.startswith(pre + 'deconv') for key in d)
    path = str(tmp_path / 'cascade.npz')
    save_npz(path, a)
    loaded = load_npz(path, b, strict=True)
    assert {'head/cascade2/score/W', 'head/cascade3/fc1/W', 'head/cascade3/conv1/W'} <= set(loaded)
    assert torch.equal(a.ps.params, b.ps.params)
    plain, c = _model(4), _model(5, cascade_ious=IOUS)
    before = {n: c.ps.p(n).clone() for n in c.ps.offsets if n.startswith('head/cascade')}
    path2 = str(tmp_path / 'plain.npz')
    save_npz(path2, plain)
    loaded = load_npz(path2, c, strict=False)
    assert not any('cascade' in k for k in loaded)
    for n in plain.ps.offsets:
        assert torch.equal(plain.ps.p(n), c.ps.p(n)), n
    assert all(torch.equal(c.ps.p(n), v) for n, v in before.items())
    with pytest.raises(KeyError):
        load_npz(path2, c, strict=True)


# ---- flags and the resume record --------------------------------------------------------------------------------------------------------
def test_flags_parse_in_all_four_scripts():
    import demo
    import evaluate
    import train
    from chainer_maskrcnn.inference_options import NO_CASCADE, cascade_flag_settings
    for parser in (train.build_parser(), train.build_parser(keypoints=True), evaluate.build_parser(), demo.build_parser()):
        a = parser.parse_args([])
        assert a.cascade == 0 and a.cascade_ious is None and a.cascade_stds is None
        a = parser.parse_args(['--cascade', '1', '--cascade-ious', '0.5', '0.6', '--cascade-stds', '0.06', '0.06', '0.12', '0.12'])
        assert a.cascade == 1 and a.cascade_ious == [0.5, 0.6] and a.cascade_stds == [0.06, 0.06, 0.12, 0.12]
        with pytest.raises(SystemExit):
            parser.parse_args(['--cascade', '2'])
    a = train.build_parser(keypoints=True).parse_args(['--cascade_ious', '0.5', '0.6', '--cascade', '1'])      # train_keypoints.py takes both spellings
    assert a.cascade_ious == [0.5, 0.6]
    assert cascade_flag_settings(0, None, None, 'fpn') == NO_CASCADE
    assert cascade_flag_settings(1, None, None, 'fpn') == {'cascade_ious': IOUS, 'cascade_stds': CASCADE_STDS}
    assert cascade_flag_settings(1, [0.5, 0.6], [0.06, 0.06, 0.12, 0.12], 'fpn_keypoint') == {
        'cascade_ious': (0.5, 0.6), 'cascade_stds': (CASCADE_STDS[0], (0.06, 0.06, 0.12, 0.12))}
    for args in ((0, [0.5, 0.6], None), (1, [0.5], None), (1, [0.5, 0.4], None), (1, None, [0.1, 0.1, 0.2])):
        with pytest.raises(ValueError, match='--cascade'):
            cascade_flag_settings(*args, 'fpn')


@pytest.mark.parametrize('arch', ['res5', 'light'])
def test_flags_refuse_the_cascade_on_the_legacy_heads(arch):
    import demo
    import evaluate
    import train
    with pytest.raises(ValueError, match='--cascade 1'):
        train.run(train.build_parser().parse_args(['--cascade', '1', '--head-arch', arch]))
    with pytest.raises(ValueError, match='--cascade 1'):
        evaluate.check_args(evaluate.build_parser().parse_args(['--cascade', '1', '--head-arch', arch]))
    with pytest.raises(ValueError, match='--cascade 1'):
        demo.check_args(demo.build_parser().parse_args(['--synthetic', '1', '--cascade', '1', '--head-arch', arch]))
    with pytest.raises(ValueError, match='--cascade 1'):
        evaluate.check_args(evaluate.build_parser().parse_args(['--cascade', '1', '--tta-hflip', '1']))


def test_resume_with_another_cascade_is_refused(tmp_path):
    import train
    from chainer_maskrcnn.inference_options import EXTENSIONS, check_resume, extension_settings
    e = {x.name: x for x in EXTENSIONS}['cascade']

    def run_settings(args):
        return extension_settings(args, '--eval-tta-', training=True)['cascade']

    def check(resume, args, path=''):
        check_resume(resume, e.state_key, e.off, run_settings(args), e.settings_noun, path)
    p = train.build_parser()
    on, off = p.parse_args(['--cascade', '1']), p.parse_args([])
    state = {'cascade': run_settings(on)}
    assert state['cascade'] == {'cascade_ious': [0.5, 0.6, 0.7], 'cascade_stds': [list(s) for s in CASCADE_STDS]}
    ck = str(tmp_path / 'trainer_5.pt')
    torch.save(dict(state, iteration=5), ck)                              # what trainer_<it>.pt records survives the file
    state = torch.load(ck, map_location='cpu', weights_only=False)
    check(state, on, ck)
    check({}, off)                                                    # a state from before the key existed: one stage
    for resume, args in ((state, off), ({}, on), (state, p.parse_args(['--cascade', '1', '--cascade-ious', '0.5', '0.6']))):
        with pytest.raises(ValueError, match='--resume .* cascade'):
            check(resume, args, ck)
    old = str(tmp_path / 'trainer_old.pt')
    torch.save({'iteration': 3}, old)
    with pytest.raises(ValueError, match='--resume .* cascade'):          # through run(): refused before any device work
        train.run(p.parse_args(['--resume', old, '--cascade', '1']))
    with pytest.raises(ValueError, match='--resume .* cascade'):
        train.run(p.parse_args(['--resume', ck]))


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_new_symbols_with_the_wrappers_argument_counts():
    sig = _hip.SIGNATURES
    assert len(sig['mrcnn_cascade_refine_f32'][1]) == 25 and len(sig['mrcnn_cascade_prob_f32'][1]) == 10
    src = open(os.path.join(ROOT, 'chainer-maskrcnn_amd', 'chainer_maskrcnn', '_hip', 'ops.py')).read()
    for name, n in (('mrcnn_cascade_refine_f32', 25), ('mrcnn_cascade_prob_f32', 10)):
        call = src[src.index('lib().' + name + '('):]
        depth, args, i = 0, 1, call.index(name) + len(name)
        for j, ch in enumerate(call[i:]):
            depth += ch in '([{'
            depth -= ch in ')]}'
            args += (ch == ',' and depth == 1)
            if depth == 0:
                break
        assert args == n, (name, args)
    assert _hip.ABI_VERSION == 10
    hip = open(os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc', 'cascade.hip')).read()
    assert len(re.findall(r'extern "C" int (mrcnn_cascade_\w+)', hip)) == 2


def test_entry_points_refuse_bad_arguments_without_a_device():
    import ctypes
    lib = _hip.lib()
    A = ctypes.c_void_p(8192)               # an address that is compared, never dereferenced
    m4 = (ctypes.c_float * 4)(0, 0, 0, 0)
    s4 = (ctypes.c_float * 4)(0.1, 0.1, 0.2, 0.2)
    M, S4 = ctypes.cast(m4, ctypes.c_void_p), ctypes.cast(s4, ctypes.c_void_p)

    def refine(rois=A, box=A, ld=88, loc0=84, N=2, S=8, mean=M, sp=S4, gt=None, gl=None, ng=None, cap=0, sn=None, roi=A, xy5=A, lev=A, loc=None,
               lab=None, asg=None):
        return lib.mrcnn_cascade_refine_f32(rois, box, ld, loc0, None, N, S, mean, sp, None, 10.0, 10.0, gt, gl, ng, cap, 0.6, sn, roi, xy5, lev, loc,
                                            lab, asg, None)
    train = dict(gt=A, gl=A, ng=A, cap=4, sn=S4, loc=A, lab=A, asg=A)
    for kw in (dict(rois=None), dict(box=None), dict(roi=None), dict(xy5=None), dict(lev=None), dict(mean=None), dict(sp=None), dict(ld=87),
               dict(loc0=-1), dict(N=-1), dict(S=-1), dict(N=70000), dict(gl=A), dict(lab=A), dict(train, gl=None), dict(train, sn=None),
               dict(train, loc=None), dict(train, cap=0)):
        assert refine(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert refine(**dict(train, cap=257)) == -2 and b'257' in lib.mrcnn_last_error()
    assert refine(N=0) == 0 and refine(S=0) == 0 and refine(**dict(train, S=0)) == 0          # nothing to do: no launch

    def prob(o=(A, A, None, None), K=2, R=4, ld=88, nc=81, out=A):
        return lib.mrcnn_cascade_prob_f32(*o, K, R, ld, nc, out, None)
    for kw in (dict(K=1), dict(K=5), dict(o=(A, None, None, None)), dict(o=(A, A, None, None), K=3), dict(R=-1), dict(nc=0), dict(ld=80), dict(out=None)):
        assert prob(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert prob(R=0) == 0


def test_ops_have_no_cpu_fallback():
    with pytest.raises(_hip.MrcnnHipError):
        ops.cascade_refine(torch.zeros((4, 4)), torch.zeros((4, 88)), 84, 1, cr.MEAN, cr.STDS[0], (10., 10.))
    with pytest.raises(_hip.MrcnnHipError):
        ops.cascade_prob([torch.zeros((4, 88)), torch.zeros((4, 88))], 81)
