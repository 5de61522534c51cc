"""Mask Scoring R-CNN without a device: the NumPy restatements of tests/maskiou_reference.py on hand-computed
cases and on the cases the GPU tests use, the model's and the scripts' refusals, the parameter layout, the NPZ link paths and the argument
errors of the new entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from chainer_maskrcnn import _hip
from chainer_maskrcnn._hip import ops
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss, mask_iou_weight_setting
from chainer_maskrcnn.model.maskrcnn import MaskRCNN, mask_iou_setting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskiou_reference as mr  # noqa: E402

SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
EPS32 = float(np.finfo(np.float32).eps)
CASES = mr.target_cases()


def _model(seed=3, **kw):
    return MaskRCNN(n_fg_class=5, device='cpu', seed=seed, _test_shrink=SHRINK, **kw)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------
def test_target_rule_by_hand():
    # (full, crop, pred, gt28, ovr): full_est = 4 * 10 / 5 = 8, uni = 3 + 8 - 2 = 9, target 2 / 9
    counts = np.array([[10, 5, 3, 4, 2], [10, 0, 3, 4, 2], [0, 5, 3, 4, 2], [7, 7, 6, 6, 6], [9, 3, 0, 5, 0], [1000, 10, 0, 0, 0]], np.int64)
    t64, t32 = mr.target_from_counts(counts, np.float64), mr.target_from_counts(counts, np.float32)
    assert t32.dtype == np.float32 and t64.dtype == np.float64
    np.testing.assert_array_equal(t64, [2 / 9, 0, 0, 1.0, 0, 0])
    np.testing.assert_array_equal(t32, np.array([np.float32(2) / np.float32(9), 0, 0, 1, 0, 0], np.float32))


def test_counts_by_hand():
    masks = np.zeros((1, 2, 6, 8), np.uint8)
    masks[0, 0, 1:5, 2:6] = 7                           # 16 nonzero bytes
    masks[0, 1] = 255                                   # beyond n_gt: never counted
    gt = np.zeros((1, 28, 28), np.int32)
    gt[0, :14] = 1                                      # 392 positions
    logit = np.full((1, 28, 28, 32), -1.0, np.float32)
    logit[0, 7:21, :, 2] = 0.5                          # 392 positions, 196 shared with gt
    logit[0, 0, 0, 2] = 0.0                             # a zero logit is no prediction
    c = dict(masks=masks, n_gt=np.array([1], np.int32), sample_roi=np.array([[0.9, 3.99, 3.2, 20.0]], np.float32), gt_assign=np.array([0], np.int32),
             label=np.array([3], np.int32), n_pos=np.array([1], np.int32), n_sample=1, rows=1, mask_out=logit, gt_roi_mask=gt)
    np.testing.assert_array_equal(mr.mask_areas(masks, c['n_gt']), [[16, 0]])
    assert mr.crop_rect(c['sample_roi'][0], 6, 8) == (0, 3, 3, 8)       # truncation, clipped to the image
    np.testing.assert_array_equal(mr.target_counts(c), [[16, 2 * 3, 392, 392, 196]])        # rows 1..2, columns 3..5 of the mask
    want = 196.0 / (392 + 392 * 16 / 6.0 - 196)
    assert mr.target(c)[0] == want
    for kw in (dict(n_pos=np.array([0], np.int32)), dict(label=np.array([0], np.int32)), dict(gt_assign=np.array([-1], np.int32)),
               dict(gt_assign=np.array([1], np.int32)), dict(sample_roi=np.array([[2.1, 0, 2.9, 8]], np.float32)),
               dict(sample_roi=np.array([[5.0, 0.0, 6.0, 8.0]], np.float32))):
        assert mr.target(dict(c, **kw))[0] == 0, kw
    assert mr.target(dict(c, label=np.array([2], np.int32)), label_base=0)[0] == want          # predict's 0-based labels


def test_input_l2_and_rescore_by_hand():
    feat = np.arange(2 * 14 * 14 * 4, dtype=np.float32).reshape(2, 14, 14, 4)
    m = np.zeros((2, 28, 28, 32), np.float32)
    m[0, 2, 4, 1], m[0, 3, 5, 1], m[0, 3, 4, 1] = 3.0, -1.0, 5.0           # the window of output (1, 2)
    m[0, 0:2, 0:2, 1] = [[-4.0, -2.0], [-3.0, -5.0]]                       # an all-negative window keeps its largest
    m[1, :, :, 0] = 9.0
    x = mr.input_fwd(feat, m, np.array([2, 0], np.int32), 36)
    assert x.shape == (2, 14, 14, 36) and x.dtype == np.float32
    np.testing.assert_array_equal(x[..., :4], feat)
    assert x[0, 1, 2, 4] == 5.0 and x[0, 0, 0, 4] == -2.0 and x[0, 5, 5, 4] == 0.0
    assert not x[1, :, :, 4].any() and not x[..., 5:].any()               # a background row has no logit channel
    assert (mr.input_fwd(feat, m, np.array([1, 0], np.int32), 36, label_base=0)[1, :, :, 4] == 9.0).all()
    g_pool = np.ones((2, 14, 14, 4), np.float32)
    g = mr.input_bwd(x, g_pool)
    np.testing.assert_array_equal(g, feat + 1)
    # the loss: rows 0 and 2 count (row 1's target is 0, row 3 is background)
    pred = np.array([[0.0, 0.5, 9.0], [1.0, 1.0, 1.0], [0.25, 7.0, 7.0], [3.0, 3.0, 3.0]], np.float32)
    loss, count, gx = mr.l2(pred, np.array([0.75, 0.0, 0.5, 0.9]), np.array([2, 1, 1, 0]), weight=2.0)
    assert count == 2 and loss == 2.0 * (0.5 * 0.25 ** 2 + 0.5 * 0.25 ** 2) / 2
    np.testing.assert_array_equal(gx, [[0, -0.25, 0], [0, 0, 0], [-0.25, 0, 0], [0, 0, 0]])
    loss, count, gx = mr.l2(pred, np.zeros(4), np.array([2, 1, 1, 0]))
    assert loss == 0 and count == 1 and not gx.any()                    # no row with a target: loss 0, zero gradient
    s = mr.rescore(np.array([0.5, 0.5, 0.5, 0.25], np.float32), np.array([[0.5, 2.0], [-1.0, 0.3], [0.1, 1.5], [1.0, 0.0]], np.float32), [0, 0, 1, 0])
    np.testing.assert_array_equal(s, np.array([0.25, 0.0, 0.5, 0.25], np.float32))


@pytest.mark.parametrize('name,case', CASES, ids=[c[0] for c in CASES])
def test_reference_targets_are_ious(name, case):
    """Before any GPU run: the reference alone gives 0 <= target <= 1 on every row of every case the GPU tests use, a positive target on at
    least half of the live random rows, and a float32 restatement within the bound test_maskiou_gpu.py derives (4.5 eps32 of the target)."""
    counts = mr.target_counts(case)
    t64, t32 = mr.target_from_counts(counts, np.float64), mr.target_from_counts(counts, np.float32)
    assert ((t64 >= 0) & (t64 <= 1)).all() and ((t32 >= 0) & (t32 <= 1)).all()
    assert (counts[:, 0] >= counts[:, 1]).all() and (counts[:, 4] <= np.minimum(counts[:, 2], counts[:, 3])).all()
    assert (np.abs(t32.astype(np.float64) - t64) <= 4.5 * EPS32 * t64).all()
    rows, n_pos = case['rows'], case['n_pos']
    live = np.concatenate([np.arange(rows) < n_pos[i] for i in range(len(n_pos))])
    assert not t64[~live].any() and not counts[~live].any()
    if name.startswith('random'):
        assert live.sum() >= 6 and (t64[live] > 0).sum() * 2 >= live.sum(), (live.sum(), (t64[live] > 0).sum())
        assert len(np.unique(t64[live])) > live.sum() // 2


def test_edge_rows_of_the_reference():
    for H, W in ((37, 45), (64, 64)):
        for n_fg in (3, 80):
            c = mr.edge_case(H, W, n_fg)
            counts, t = mr.target_counts(c), mr.target(c)
            z = mr.target_counts(mr.edge_case(H, W, n_fg, junk=0))
            np.testing.assert_array_equal(counts, z)            # what the unused mask slots hold does not matter
            row = dict(zip(mr.EDGE_ROWS, range(12)))
            full0 = 15 * 23 - 16
            assert counts[row['partly outside']][0] == full0 and 0 < counts[row['partly outside']][1] < full0 and t[row['partly outside']] > 0
            assert counts[row['no integer extent']][1] == 0 and t[row['no integer extent']] == 0
            assert counts[row['the image']][1] == full0 and t[row['the image']] > 0
            assert counts[row['all-zero mask']][0] == 0 and t[row['all-zero mask']] == 0
            assert counts[row['crop 0, full > 0']][:2].tolist() == [full0, 0] and t[row['crop 0, full > 0']] == 0
            assert counts[row['all logits negative']][2] == 0 and counts[row['all logits negative']][3] > 0 and t[row['all logits negative']] == 0
            e = counts[row['exact one']]
            assert e[0] == e[1] and e[2] == e[3] == e[4] > 0 and t[row['exact one']] == 1.0
            assert mr.target(c, dtype=np.float32)[row['exact one']] == np.float32(1.0)
            assert c['label'][row['last channel']] == n_fg and counts[row['last channel']][1] == 9 * 11 and t[row['last channel']] > 0
            assert t[row['ordinary']] > 0
            assert not counts[9:].any() and not t[9:].any()             # behind n_pos, no assignment, background, the image without positives


# ---- the model and the chain --------------------------------------------------------------------------------------------------------------
def test_settings_and_their_refusals():
    assert mask_iou_setting(False) is False and mask_iou_setting(True) is True and mask_iou_setting(0, 'res5') is False
    for arch in ('fpn_keypoint', 'res5', 'light'):
        with pytest.raises(ValueError, match='mask_iou'):
            mask_iou_setting(True, arch)
    with pytest.raises(ValueError, match='mask_iou'):
        mask_iou_setting('yes')
    assert mask_iou_weight_setting(2) == 2.0
    for w in (0, -1.0, float('nan'), float('inf'), True, '1', None):
        with pytest.raises(ValueError, match='mask_iou_weight'):
            mask_iou_weight_setting(w)
    with pytest.raises(ValueError, match='mask_iou'):
        MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', device='cpu', _test_shrink=SHRINK, mask_iou=True)
    with pytest.raises(ValueError, match='mask_iou'):
        MaskRCNN(n_fg_class=5, backbone='c4', head_arch='res5', device='cpu', _test_shrink=dict(width_div=4), mask_iou=True)
    m = _model(mask_iou=True)
    with pytest.raises(ValueError, match='mask_iou_weight'):
        FPNMaskRCNNTrainChain(m, mask_iou_weight=0.0)
    with pytest.raises(ValueError, match='mask_loss_fun'):         # a generic loss function re-orders the mask rows
        FPNMaskRCNNTrainChain(m, mask_loss_fun=lambda x, y, xp, l: x.sum())
    assert FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, mask_iou_weight=0.5).mask_iou_weight == 0.5
    with pytest.raises(ValueError, match='mask_iou'):
        m.use_test_augmentation([160, 200])
    assert m.tta is None and m.mask_iou_rescore is True
    FPNMaskRCNNTrainChain(_model(), mask_loss_fun=lambda x, y, xp, l: x.sum())        # without the head a generic loss stays allowed


def test_head_adds_only_its_own_parameters_behind_every_other():
    plain, off = _model(), _model(mask_iou=False)
    assert plain.ps.offsets == off.ps.offsets and list(plain.ps.offsets) == list(off.ps.offsets) and torch.equal(plain.ps.params, off.ps.params)
    assert plain.maskiou_head is None and plain.head.keep_mask_pool is False
    layers = ['conv1', 'conv2', 'conv3', 'conv4', 'fc1', 'fc2', 'maskiou']
    own = ['head/maskiou/%s/%s' % (l, p) for l in layers for p in ('W', 'b')]
    for kw in ({}, dict(cascade_ious=(0.5, 0.6, 0.7)), dict(head_norm='gn', gn_groups=16)):
        base, m = _model(**kw), _model(mask_iou=True, **kw)
        assert [n for n in m.ps.offsets if n not in base.ps.offsets] == own
        assert list(m.ps.offsets)[:len(base.ps.offsets)] == list(base.ps.offsets)           # behind the cascade's stages too
        for n in base.ps.offsets:       # every other parameter keeps its offset, its shape and its draw from the initialisation stream
            assert m.ps.offsets[n] == base.ps.offsets[n], n
            assert torch.equal(m.ps.p(n), base.ps.p(n)), n
        end = max(o + int(np.prod(s)) for o, s in base.ps.offsets.values())
        assert all(m.ps.offsets[n][0] >= end for n in own)
        assert not any('/gn/' in n for n in own)                # plain conv + ReLU whatever head_norm is
    h = m.maskiou_head
    c = m.head.channels
    assert m.ps.offsets['head/maskiou/conv1/W'][1] == (c, 3, 3, c + 32) and h.cin_p == c + 32 and h.conv1.cin == c + 1
    assert h.conv4.stride == 2 and h.out_size == 7 and m.ps.offsets['head/maskiou/fc1/W'][1] == (h.fc1.cout_p, 1, 1, 49 * c)
    assert h.out.cout == m.n_class - 1 == 5 and h.out_p == 32
    for n in own[::2]:
        w = m.ps.p(n)
        assert float(w.abs().max()) > 0, n
    assert not m.ps.p('head/maskiou/conv1/W')[:, :, :, c + 1:].any() and float(m.ps.p('head/maskiou/conv1/W')[:, :, :, c].abs().max()) > 0


def test_npz_link_paths_and_round_trip(tmp_path):
    from chainer_maskrcnn.utils.chainer_npz import ChainerNpzMap, load_npz, save_npz
    a, b = _model(1, mask_iou=True, cascade_ious=(0.5, 0.6)), _model(2, mask_iou=True, cascade_ious=(0.5, 0.6))
    for n in a.ps.offsets:
        if n.startswith('head/maskiou') and n.endswith('/b'):
            a.ps.p(n)[:3] = torch.tensor([0.5, -1.0, 2.0])
    d = ChainerNpzMap(a).to_chainer()
    h, c = a.maskiou_head, a.head.channels
    pre = 'head/maskiou/'
    assert sorted(k for k in d if k.startswith(pre)) == sorted(pre + '%s/%s' % (l, p) for l in ('conv1', 'conv2', 'conv3', 'conv4', 'fc1', 'fc2', 'maskiou')
                                                                for p in ('W', 'b'))
    assert d[pre + 'conv1/W'].shape == (c, c + 1, 3, 3) and d[pre + 'conv4/W'].shape == (c, c, 3, 3) and d[pre + 'conv2/b'].shape == (c,)
    assert d[pre + 'fc1/W'].shape == (h.fc1.cout, c * 49) and d[pre + 'fc2/W'].shape == (h.fc2.cout, h.fc2.cin)
    assert d[pre + 'maskiou/W'].shape == (5, h.fc2.cout) and d[pre + 'maskiou/b'].shape == (5,)
    # fc1: Chainer's Linear flattens (c, h, w), the store (h, w, c) - the permutation of the box head's fc1
    w = a.ps.p(pre + 'fc1/W').numpy()[:h.fc1.cout, 0, 0, :].reshape(-1, 7, 7, c)
    np.testing.assert_array_equal(d[pre + 'fc1/W'].reshape(-1, c, 7, 7), w.transpose(0, 3, 1, 2))
    path = str(tmp_path / 'maskiou.npz')
    save_npz(path, a)
    loaded = load_npz(path, b, strict=True)
    assert {pre + 'conv1/W', pre + 'fc1/W', pre + 'fc1/b', pre + 'maskiou/W', pre + 'conv4/b'} <= set(loaded)
    assert torch.equal(a.ps.params, b.ps.params)
    plain, cm = _model(4), _model(5, mask_iou=True)
    before = {n: cm.ps.p(n).clone() for n in cm.ps.offsets if n.startswith('head/maskiou')}
    path2 = str(tmp_path / 'plain.npz')
    save_npz(path2, plain)
    loaded = load_npz(path2, cm, strict=False)
    assert not any('maskiou' in k for k in loaded)
    for n in plain.ps.offsets:
        assert torch.equal(plain.ps.p(n), cm.ps.p(n)), n
    assert all(torch.equal(cm.ps.p(n), v) for n, v in before.items())
    with pytest.raises(KeyError):
        load_npz(path2, cm, strict=True)
    assert sorted(ChainerNpzMap(plain).to_chainer()) == sorted(k for k in d if 'maskiou' not in k and 'cascade' not in k)


# ---- flags and the resume record ----------------------------------------------------------------------------------------------------------
def test_flags_in_the_four_scripts():
    import demo
    import evaluate
    import train
    from chainer_maskrcnn.inference_options import NO_MASK_IOU, mask_iou_settings
    for parser in (train.build_parser(), train.build_parser(keypoints=True), evaluate.build_parser(), demo.build_parser()):
        assert parser.parse_args([]).mask_iou == 0 and parser.parse_args(['--mask-iou', '1']).mask_iou == 1
        with pytest.raises(SystemExit):
            parser.parse_args(['--mask-iou', '2'])
    a = train.build_parser().parse_args(['--mask-iou', '1', '--mask-iou-weight', '0.5'])
    assert a.mask_iou_weight == 0.5 and train.build_parser().parse_args([]).mask_iou_weight is None
    for parser in (evaluate.build_parser(), demo.build_parser()):          # the weight is a training flag
        with pytest.raises(SystemExit):
            parser.parse_args(['--mask-iou-weight', '0.5'])
    assert train.build_parser(keypoints=True).parse_args(['--mask_iou', '1']).mask_iou == 1          # train_keypoints.py takes both spellings
    assert mask_iou_settings(0) == NO_MASK_IOU == {'mask_iou': False, 'mask_iou_weight': 1.0}
    assert mask_iou_settings(1) == {'mask_iou': True, 'mask_iou_weight': 1.0}
    assert mask_iou_settings(1, 0.25) == {'mask_iou': True, 'mask_iou_weight': 0.25}
    for args in ((0, 0.5), (1, 0.0), (1, float('nan')), (2, None)):
        with pytest.raises(ValueError, match='--mask-iou'):
            mask_iou_settings(*args)
    for arch in ('res5', 'light', 'fpn_keypoint'):
        with pytest.raises(ValueError, match='--mask-iou 1'):
            mask_iou_settings(1, None, arch)


def test_scripts_refuse_what_the_model_refuses():
    import demo
    import evaluate
    import train
    for arch in ('res5', 'light'):
        with pytest.raises(ValueError, match='--mask-iou 1'):
            train.run(train.build_parser().parse_args(['--mask-iou', '1', '--head-arch', arch]))
        with pytest.raises(ValueError, match='--mask-iou 1'):
            evaluate.check_args(evaluate.build_parser().parse_args(['--mask-iou', '1', '--head-arch', arch]))
        with pytest.raises(ValueError, match='--mask-iou 1'):
            demo.check_args(demo.build_parser().parse_args(['--synthetic', '1', '--mask-iou', '1', '--head-arch', arch]))
    with pytest.raises(ValueError, match='--mask-iou'):              # train_keypoints.py refuses the flag
        train.run(train.build_parser(keypoints=True).parse_args(['--mask-iou', '1']), keypoints=True)
    with pytest.raises(ValueError, match='--mask-iou'):
        train.run(train.build_parser(keypoints=True).parse_args(['--mask-iou-weight', '2']), keypoints=True)
    # test-time augmentation is refused before the model is built
    with pytest.raises(ValueError, match='--mask-iou 1 .*tta'):
        evaluate.check_args(evaluate.build_parser().parse_args(['--mask-iou', '1', '--tta-hflip', '1']))
    with pytest.raises(ValueError, match='--mask-iou 1 .*tta'):
        demo.check_args(demo.build_parser().parse_args(['--synthetic', '1', '--mask-iou', '1', '--tta-sizes', '160', '200']))
    with pytest.raises(ValueError, match='--mask-iou 1 .*eval-tta'):
        train.run(train.build_parser().parse_args(['--mask-iou', '1', '--eval-tta-hflip', '1']))
    with pytest.raises(ValueError, match='--mask-iou-weight belongs'):
        train.run(train.build_parser().parse_args(['--mask-iou-weight', '2']))


def test_resume_with_another_setting_is_refused(tmp_path):
    import train
    p = train.build_parser()
    from chainer_maskrcnn.inference_options import EXTENSIONS, check_resume, extension_settings
    e = {x.name: x for x in EXTENSIONS}['mask_iou']

    def run_settings(args):
        return extension_settings(args, '--eval-tta-', training=True)['mask_iou']

    def check(resume, args, path=''):
        check_resume(resume, e.state_key, e.off, run_settings(args), e.settings_noun, path)
    on, off, half = p.parse_args(['--mask-iou', '1']), p.parse_args([]), p.parse_args(['--mask-iou', '1', '--mask-iou-weight', '0.5'])
    state = {'mask_iou': run_settings(on)}
    assert state['mask_iou'] == {'mask_iou': True, 'mask_iou_weight': 1.0}
    ck = str(tmp_path / 'trainer_5.pt')
    torch.save(dict(state, iteration=5), ck)
    state = torch.load(ck, map_location='cpu', weights_only=False)
    check(state, on, ck)
    check({}, off)                                    # a state from before the key existed: no MaskIoU head
    for resume, args in ((state, off), ({}, on), (state, half)):
        with pytest.raises(ValueError, match='--resume .* Mask Scoring'):
            check(resume, args, ck)
    old = str(tmp_path / 'trainer_old.pt')
    torch.save({'iteration': 3}, old)
    with pytest.raises(ValueError, match='--resume .* Mask Scoring'):          # through run(): refused before any device work
        train.run(p.parse_args(['--resume', old, '--mask-iou', '1']))
    with pytest.raises(ValueError, match='--resume .* Mask Scoring'):
        train.run(p.parse_args(['--resume', ck]))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
NEW = {'mrcnn_maskiou_target_workspace_bytes': 2, 'mrcnn_maskiou_target': 24, 'mrcnn_maskiou_input_fwd': 12, 'mrcnn_maskiou_input_bwd': 7,
       'mrcnn_maskiou_l2': 13, 'mrcnn_maskiou_rescore': 8}


def test_abi_declares_the_new_symbols_with_the_wrappers_argument_counts():
    sig = _hip.SIGNATURES
    src = open(os.path.join(ROOT, 'chainer-maskrcnn_amd', 'chainer_maskrcnn', '_hip', 'ops.py')).read()
    for name, n in NEW.items():
        assert len(sig[name][1]) == n, name
        call = src[src.index('lib().' + name + '('):]
        depth, args, i = 0, 1, call.index(name) + len(name)
        for ch in call[i:]:
            depth += ch in '([{'
            depth -= ch in ')]}'
            args += (ch == ',' and depth == 1)
            if depth == 0:
                break
        assert args == n, (name, args)
    assert _hip.ABI_VERSION == 10 and _hip.lib().mrcnn_abi_version() == 10
    hip = open(os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc', 'maskiou.hip')).read()
    assert sorted(re.findall(r'extern "C" (?:int|size_t) (mrcnn_maskiou_\w+)', hip)) == sorted(NEW)
    assert 'atomicAdd' not in hip and 'asm(' not in hip and 'asm volatile' not in hip          # plain HIP C++, no atomics of any kind


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _hip.lib()
    A = ctypes.c_void_p(8192)               # an address that is compared, never dereferenced
    assert lib.mrcnn_maskiou_target_workspace_bytes(2, 4) == 2 * 4 * 32 * 4 and lib.mrcnn_maskiou_target_workspace_bytes(0, 4) == 0

    def target(masks=A, N=2, G=4, H=37, W=45, n_gt=A, roi=A, asg=A, lab=A, n_pos=A, S=12, rows=12, mo=A, msz=28, Cp=32, nch=3, gm=A, base=1, area=A,
               tgt=A, counts=None, ws=A, wsb=4096):
        return lib.mrcnn_maskiou_target(masks, N, G, H, W, n_gt, roi, asg, lab, n_pos, S, rows, mo, msz, Cp, nch, gm, base, area, tgt, counts, ws, wsb,
                                        None)
    for kw in (dict(masks=None), dict(n_gt=None), dict(roi=None), dict(asg=None), dict(lab=None), dict(n_pos=None), dict(mo=None), dict(gm=None),
               dict(area=None), dict(tgt=None), dict(ws=None), dict(N=0), dict(G=0), dict(H=0), dict(W=-1), dict(S=0), dict(rows=-1), dict(rows=13),
               dict(msz=0), dict(Cp=0), dict(nch=0), dict(nch=33), dict(nch=81, Cp=64)):
        assert target(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert target(wsb=16) != 0 and b'workspace' in lib.mrcnn_last_error()
    assert target(rows=0) == 0 and target(rows=0, masks=None, tgt=None) == 0           # no rows: nothing to do, no launch

    def fwd(feat=A, mo=A, lab=A, base=1, Rm=4, P=14, C=64, Cp=32, nch=3, cin_p=96, out=A):
        return lib.mrcnn_maskiou_input_fwd(feat, mo, lab, base, Rm, P, C, Cp, nch, cin_p, out, None)
    for kw in (dict(feat=None), dict(mo=None), dict(lab=None), dict(out=None), dict(Rm=-1), dict(P=0), dict(C=0), dict(C=62), dict(cin_p=64),
               dict(cin_p=66), dict(Cp=0), dict(nch=0), dict(nch=33)):
        assert fwd(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert fwd(Rm=0) == 0 and fwd(Rm=0, feat=None) == 0

    def bwd(g_in=A, Rm=4, P=14, C=64, cin_p=96, g_pool=A):
        return lib.mrcnn_maskiou_input_bwd(g_in, Rm, P, C, cin_p, g_pool, None)
    for kw in (dict(g_in=None), dict(g_pool=None), dict(Rm=-1), dict(P=0), dict(C=0), dict(C=30), dict(cin_p=32), dict(cin_p=0)):
        assert bwd(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert bwd(Rm=0) == 0

    def l2(pred=A, ld=32, nch=3, tgt=A, lab=A, base=1, Rm=4, w=1.0, out=A, gx=A, ws=A, wsb=1 << 20):
        return lib.mrcnn_maskiou_l2(pred, ld, nch, tgt, lab, base, Rm, w, out, gx, ws, wsb, None)
    for kw in (dict(pred=None), dict(tgt=None), dict(lab=None), dict(out=None), dict(ws=None), dict(Rm=-1), dict(ld=0), dict(nch=0), dict(nch=33),
               dict(w=0.0), dict(w=-1.0), dict(w=float('nan')), dict(w=float('inf'))):
        assert l2(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert l2(wsb=16) != 0 and b'workspace' in lib.mrcnn_last_error()

    def rescore(score=A, pred=A, ld=32, nch=3, lab=A, D=4, out=A):
        return lib.mrcnn_maskiou_rescore(score, pred, ld, nch, lab, D, out, None)
    for kw in (dict(score=None), dict(pred=None), dict(lab=None), dict(out=None), dict(D=-1), dict(ld=0), dict(nch=0), dict(nch=33)):
        assert rescore(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert rescore(D=0) == 0 and rescore(D=0, score=None) == 0


def test_ops_have_no_cpu_fallback():
    i32 = torch.int32
    with pytest.raises(_hip.MrcnnHipError):
        ops.maskiou_input_fwd(torch.zeros((1, 14, 14, 64)), torch.zeros((1, 28, 28, 32)), torch.zeros((1,), dtype=i32), 3, 96)
    with pytest.raises(_hip.MrcnnHipError):
        ops.maskiou_input_bwd(torch.zeros((1, 14, 14, 96)), torch.zeros((1, 14, 14, 64)))
    with pytest.raises(_hip.MrcnnHipError):
        ops.maskiou_l2(torch.zeros((2, 32)), torch.zeros((2,)), torch.zeros((2,), dtype=i32), 3)
    with pytest.raises(_hip.MrcnnHipError):
        ops.maskiou_rescore(torch.zeros((2,)), torch.zeros((2, 32)), torch.zeros((2,), dtype=i32), 3)
    with pytest.raises(_hip.MrcnnHipError):
        ops.maskiou_target(torch.zeros((1, 1, 8, 8), dtype=torch.uint8), torch.ones((1,), dtype=i32), torch.zeros((2, 4)), torch.zeros((2,), dtype=i32),
                           torch.zeros((2,), dtype=i32), torch.ones((1,), dtype=i32), 2, 2, torch.zeros((2, 28, 28, 32)),
                           torch.zeros((2, 28, 28), dtype=i32), 3)
