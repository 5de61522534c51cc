"""PointRend without a device: the rules of tests/pointrend_reference.py by hand, the settings and their refusals,
the parameter layout, the NPZ files, the scripts' flags, the resume record and the C entry points' argument checks."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from chainer_maskrcnn import _hip
from chainer_maskrcnn._hip import ops
from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss, point_loss_weight_setting
from chainer_maskrcnn.model.maskrcnn import MaskRCNN, point_rend_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pointrend_reference as pr  # noqa: E402

SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
F32, F64 = np.float32, np.float64


# ---- the rules by hand --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [F32, F64])
def test_point_sample_by_hand(dt):
    m = np.arange(12, dtype=np.float32).reshape(3, 4)           # m[y][x] = 4 y + x
    # interior: (px, py) = (1.75, 1.25) -> fx = 1.25, fy = 0.75: taps (0,1) (0,2) (1,1) (1,2) = 1, 2, 5, 6, weights .25*.75, .25*.25, .75*.75, .75*.25
    # two taps outside: (0.25, 1.5) -> fx = -0.25, fy = 1.0: x0 = -1 is outside, taps (1,0) = 4 with (1-0)*(.75), (2,0) = 8 with 0*(.75)
    # exactly on the centre of pixel (y, x) = (2, 3): (3.5, 2.5) -> lx = ly = 0, weight 1 on m[2][3] = 11
    got = pr.point_sample(m, np.array([1.75, 0.25, 3.5]), np.array([1.25, 1.5, 2.5]), dt)
    want = [0.1875 * 1 + 0.0625 * 2 + 0.5625 * 5 + 0.1875 * 6, 0.75 * 4, 11.0]
    np.testing.assert_array_equal(got, np.array(want, dt))
    assert got.dtype == dt
    x0, y0, w = pr.taps(np.array([3.5]), np.array([2.5]), 4, 3, dt)
    assert (x0[0], y0[0]) == (3, 2) and [float(v[0]) for v in w] == [1.0, 0.0, 0.0, 0.0]
    # far outside, and coordinates no integer holds: all taps outside, zero
    np.testing.assert_array_equal(pr.point_sample(m, np.array([-7.0, 1e30, -1e30]), np.array([1.0, 1.0, 1.0]), dt), np.zeros(3, dt))
    # channels ride along
    mc = np.stack([m, -m], -1)
    np.testing.assert_array_equal(pr.point_sample(mc, np.array([1.75]), np.array([1.25]), dt)[0], np.array([want[0], -want[0]], dt))


def test_keys_coordinates_and_frame():
    k = np.array([0, 255, 256, 0xffffffff, 0x80000000], np.uint32)
    np.testing.assert_array_equal(pr.key_unit(k), np.array([0, 0, 2.0 ** -24, 1 - 2.0 ** -24, 0.5], F32))
    np.testing.assert_array_equal(pr.key_unit(k.view(np.int32)), pr.key_unit(k))             # the wrappers carry the bits in int32
    rois = np.array([[1, 10, 20, 30, 60]], F32)
    X, Y = pr.frame(rois, np.array([[[0, 0], [0.5, 0.25]]], F32), F32)
    assert X.tolist() == [[10.0, 20.0]] and Y.tolist() == [[20.0, 30.0]]


@pytest.mark.parametrize('dt', [F32, F64])
def test_clamped_upsample_of_a_2x2_grid(dt):
    g = np.array([[0.0, 16.0], [32.0, 48.0]], np.float32)
    want = np.array([[0, 4, 12, 16], [8, 12, 20, 24], [24, 28, 36, 40], [32, 36, 44, 48]], dt)
    np.testing.assert_array_equal(pr.upsample2x(g, dt), want)              # corners equal the grid's: clamped taps, not zero padding
    up, index, coords = pr.subdivide(g[None], 3, dt)
    np.testing.assert_array_equal(up[0], want)
    assert index.tolist() == [[0, 1, 4]]                                  # |0|, |4|, |8|: cells (0,0), (0,1), (1,0), in ascending flat index
    np.testing.assert_array_equal(coords[0], np.array([[0.125, 0.125], [0.375, 0.125], [0.125, 0.375]], dt))


def test_ranking_with_ties():
    # subdivision: four cells tie at |v| = 1 behind one zero; three are taken - the zero and the two lowest flat indices of the tie
    up_of = np.array([[1.0, -1.0], [0.0, 1.0]], np.float32)
    up, index, _ = pr.subdivide(up_of[None], 3)
    flat = np.abs(up[0].reshape(-1))
    order = np.argsort(flat, kind='stable')[:3]
    assert index[0].tolist() == sorted(order.tolist()) and flat[index[0]].max() <= np.sort(flat)[2]
    _, all_of_them, _ = pr.subdivide(up_of[None], 100)
    assert all_of_them[0].tolist() == list(range(16))
    # training points: candidates 0, 2 and 3 share one position (so one uncertainty); with 2 of 4 taken the tie goes to the lower indices
    keys = np.zeros((1, 2 * 4 + 2 * 1), np.uint32)
    keys[0, 2:4] = (0x40000000, 0xc0000000)                 # candidate 1 elsewhere
    keys[0, 8:10] = (0x80000000, 0x80000000)                # the uniform remainder
    coarse = np.zeros((1, 2, 2, 32), np.float32)
    coarse[0, :, :, 1] = [[3.0, 3.0], [0.0, 0.0]]           # class 2's logits: candidates 0, 2, 3 at (0, 0) see |0.75|, candidate 1 sees |0|
    coords, picked = pr.train_coords(keys, coarse, np.array([2], np.int32), 3, 3, 4, 2)
    assert picked.tolist() == [[1, 0]]                      # the most uncertain first, then the lowest index of the tie
    np.testing.assert_array_equal(coords[0], np.array([[0.25, 0.75], [0.0, 0.0], [0.5, 0.5]], F32))
    _, picked = pr.train_coords(keys, coarse, np.array([0], np.int32), 3, 3, 4, 2)           # no class: every candidate ties
    assert picked.tolist() == [[0, 1]]


def test_target_and_loss_by_hand():
    c = pr.target_case()
    a = (c['masks'], c['n_gt'], c['rois'], c['gt_assign'], c['label'], c['n_pos'], c['n_sample'], c['rows'], c['coords'])
    t = pr.target(*a, F64)
    live = pr.live_rows(c['n_gt'], c['gt_assign'], c['label'], c['n_pos'], c['n_sample'], c['rows'], 3)
    assert (t[~live] == -1).all() and (t[live] >= 0).all() and (t[live] <= 1).all() and live.sum() == 5
    pred = np.zeros((2, 3, 32), np.float32)
    pred[0, :, 1] = (0.0, 2.0, -2.0)
    tgt = np.array([[1.0, 0.5, 0.0], [-1, -1, -1]], np.float32)
    loss, count, gx = pr.bce(pred, tgt, np.array([2, 1], np.int32), 3, 2.0)
    sp = np.log1p(np.exp(-2.0))
    assert count == 3 and loss == pytest.approx(2.0 * (np.log(2.0) + (2.0 - 1.0 + sp) + sp) / 3, rel=1e-12)
    sig = 1 / (1 + np.exp(-2.0))
    np.testing.assert_allclose(gx[0, :, 1], np.array([0.5 - 1, sig - 0.5, (1 - sig) - 0]) * 2.0 / 3, rtol=1e-12)
    gx[0, :, 1] = 0
    assert not gx.any()
    assert pr.bce(pred, np.full((2, 3), -1, np.float32), np.array([2, 1], np.int32), 3, 1.0)[:2] == (0.0, 1)


# ---- settings, refusals, parameters -------------------------------------------------------------------------------------------------------
def test_settings_and_their_refusals():
    assert point_rend_settings() is None and point_rend_settings(False) is None
    st = point_rend_settings(True)
    assert st == dict(train_points=196, oversample=3, importance=0.75, n_candidates=588, n_important=147, subdivision_steps=2,
                      subdivision_points=784)
    assert point_rend_settings(True, 8, 3, 0.75)['n_important'] == 6
    for kw, word in ((dict(head_arch='fpn_keypoint'), 'keypoint'), (dict(head_arch='res5'), 'head_arch'), (dict(head_arch='light'), 'head_arch'),
                     (dict(mask_iou=True), 'mask_iou'), (dict(point_train_points=0), 'point_train_points'),
                     (dict(point_oversample=0), 'point_oversample'), (dict(point_oversample=2.5), 'point_oversample'),
                     (dict(point_importance=1.5), 'point_importance'), (dict(point_importance=-0.1), 'point_importance'),
                     (dict(subdivision_steps=0), 'subdivision_steps'), (dict(subdivision_steps=3), 'subdivision_steps'),
                     (dict(subdivision_points=0), 'subdivision_points'), (dict(point_train_points=2000), 'point_oversample')):
        with pytest.raises(ValueError, match=word):
            point_rend_settings(True, **kw)
    with pytest.raises(ValueError, match='point_rend'):
        point_rend_settings('yes')
    assert point_loss_weight_setting(2) == 2.0
    for w in (0, -1.0, float('nan'), float('inf'), True, '1'):
        with pytest.raises(ValueError, match='point_loss_weight'):
            point_loss_weight_setting(w)
    with pytest.raises(ValueError, match='point_rend'):
        MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', device='cpu', _test_shrink=SHRINK, point_rend=True)
    with pytest.raises(ValueError, match='point_rend together with mask_iou'):
        MaskRCNN(n_fg_class=5, device='cpu', _test_shrink=SHRINK, point_rend=True, mask_iou=True)
    m = MaskRCNN(n_fg_class=5, device='cpu', _test_shrink=SHRINK, point_rend=True)
    with pytest.raises(ValueError, match='use_test_augmentation.*point_rend'):
        m.use_test_augmentation([160, 200])
    with pytest.raises(ValueError, match='point_rend.*mask_loss_fun'):
        FPNMaskRCNNTrainChain(m, mask_loss_fun=lambda *a: None)
    with pytest.raises(ValueError, match='point_loss_weight'):
        FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, point_loss_weight=0)
    chain = FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, point_loss_weight=0.5)
    assert chain.point_loss_weight == 0.5 and chain.point_keys is None
    assert m.point_rend_refine is True and m.last_point_grid is None


@pytest.mark.parametrize('kw', [{}, dict(cascade_ious=(0.5, 0.6, 0.7)), dict(head_norm='gn', gn_groups=16)], ids=['plain', 'cascade', 'gn'])
def test_head_adds_only_its_own_parameters_behind_every_other(kw):
    plain = MaskRCNN(n_fg_class=5, device='cpu', seed=3, _test_shrink=SHRINK, **kw)
    m = MaskRCNN(n_fg_class=5, device='cpu', seed=3, _test_shrink=SHRINK, point_rend=True, **kw)
    assert plain.point_head is None and plain.point_rend is None
    names, pnames = m.ps.names(), plain.ps.names()
    own = [n for n in names if n.startswith('head/point/')]
    assert own == ['head/point/%s/%s' % (l, p) for l in ('fc1', 'fc2', 'fc3', 'predictor') for p in ('W', 'b')]
    assert names == pnames + own                                    # behind every other parameter, the cascade's included
    for n in pnames:
        assert m.ps.offsets[n] == plain.ps.offsets[n]
    assert torch.equal(m.ps.params[:plain.ps.size], plain.ps.params) and m.ps.size > plain.ps.size
    ph, c = m.point_head, m.head.channels
    assert (ph.fc1.cin, ph.fc2.cin, ph.predictor.cin, ph.predictor.cout) == (c + 5, 64 + 5, 64 + 5, 5) and ph.fc_channels == 64
    w = m.ps.p('head/point/predictor/W')[:5, 0, 0, :69]
    assert 0.0005 < float(w.std()) < 0.002                          # std 0.001
    assert 0.05 < float(m.ps.p('head/point/fc2/W')[:64, 0, 0, :69].std()) < 0.25       # the default initialisation: 1 / sqrt(fan_in)
    assert not m.ps.p('head/point/fc1/W')[:, 0, 0, c + 5:].any() and not m.ps.p('head/point/fc1/b').any()
    full = MaskRCNN(n_fg_class=80, device='cpu', seed=3, _test_shrink=dict(stages=(1, 1, 1, 1)), point_rend=True).point_head
    assert (full.fc1.cin, full.fc1.cout, full.cin_p, full.fc2.cin_p, full.out_p) == (336, 256, 352, 352, 96)


def test_npz_link_paths_and_round_trip(tmp_path):
    from chainer_maskrcnn.utils.chainer_npz import ChainerNpzMap, load_npz, save_npz
    m = MaskRCNN(n_fg_class=5, device='cpu', seed=3, _test_shrink=SHRINK, point_rend=True)
    path = str(tmp_path / 'point.npz')
    save_npz(path, m)
    d = np.load(path)
    assert d['head/point/fc1/W'].shape == (64, m.head.channels + 5) and d['head/point/predictor/W'].shape == (5, 69)
    assert d['head/point/fc3/b'].shape == (64,) and d['head/point/predictor/b'].shape == (5,)
    other = MaskRCNN(n_fg_class=5, device='cpu', seed=4, _test_shrink=SHRINK, point_rend=True)
    assert not torch.equal(other.ps.params, m.ps.params)
    load_npz(path, other, strict=True)
    assert torch.equal(other.ps.params, m.ps.params)
    plain = MaskRCNN(n_fg_class=5, device='cpu', seed=5, _test_shrink=SHRINK)
    assert sorted(ChainerNpzMap(plain).to_chainer()) == sorted(k for k in d.files if not k.startswith('head/point/'))
    ppath = str(tmp_path / 'plain.npz')
    save_npz(ppath, plain)
    init = {n: other.ps.p(n).clone() for n in other.ps.names() if n.startswith('head/point/')}
    load_npz(ppath, other, strict=False)                            # a plain file fills everything but the point head
    for n, v in init.items():
        assert torch.equal(other.ps.p(n), v), n
    assert torch.equal(other.ps.params[:plain.ps.size], plain.ps.params)
    with pytest.raises(KeyError):
        load_npz(ppath, other, strict=True)


# ---- flags and the resume record ----------------------------------------------------------------------------------------------------------
SHAPE_FLAGS = ('--point-train-points', '--point-oversample', '--point-importance', '--subdivision-steps', '--subdivision-points')


def test_flags_in_the_four_scripts():
    import demo
    import evaluate
    import train
    from chainer_maskrcnn.inference_options import NO_POINT_REND, point_rend_flag_settings, point_rend_model_kwargs
    for parser in (train.build_parser(), train.build_parser(keypoints=True), evaluate.build_parser(), demo.build_parser()):
        a = parser.parse_args([])
        assert a.point_rend == 0 and parser.parse_args(['--point-rend', '1']).point_rend == 1
        assert all(getattr(a, f[2:].replace('-', '_')) is None for f in SHAPE_FLAGS)
        with pytest.raises(SystemExit):
            parser.parse_args(['--point-rend', '2'])
        b = parser.parse_args(['--point-rend', '1', '--point-train-points', '98', '--point-oversample', '2', '--point-importance', '0.5',
                               '--subdivision-steps', '1', '--subdivision-points', '400'])
        s = point_rend_flag_settings(b)
        assert (s['point_train_points'], s['point_oversample'], s['point_importance'], s['subdivision_steps'], s['subdivision_points']) == \
            (98, 2, 0.5, 1, 400) and s['point_rend'] is True and s['point_loss_weight'] == 1.0
        assert point_rend_model_kwargs(s) == {k: v for k, v in s.items() if k != 'point_loss_weight'}
        assert point_rend_flag_settings(a) == NO_POINT_REND and point_rend_model_kwargs(NO_POINT_REND) == {}
    a = train.build_parser().parse_args(['--point-rend', '1', '--point-loss-weight', '0.5'])
    assert a.point_loss_weight == 0.5 and point_rend_flag_settings(a, weight=True)['point_loss_weight'] == 0.5
    for parser in (evaluate.build_parser(), demo.build_parser()):          # the weight is a training flag
        with pytest.raises(SystemExit):
            parser.parse_args(['--point-loss-weight', '0.5'])
    assert NO_POINT_REND == dict(point_rend=False, point_loss_weight=1.0, point_train_points=196, point_oversample=3, point_importance=0.75,
                                 subdivision_steps=2, subdivision_points=784)
    p = train.build_parser()
    for argv in (['--point-train-points', '98'], ['--subdivision-points', '5'], ['--point-loss-weight', '2']):
        with pytest.raises(ValueError, match='belongs to --point-rend 1'):
            point_rend_flag_settings(p.parse_args(argv), weight=True)
    for argv in (['--point-rend', '1', '--point-loss-weight', '0'], ['--point-rend', '1', '--subdivision-steps', '3'],
                 ['--point-rend', '1', '--point-importance', '2']):
        with pytest.raises(ValueError, match='--point-rend 1'):
            point_rend_flag_settings(p.parse_args(argv), weight=True)


def test_scripts_refuse_what_the_model_refuses():
    import demo
    import evaluate
    import train
    for arch in ('res5', 'light'):
        with pytest.raises(ValueError, match='--point-rend 1'):
            train.run(train.build_parser().parse_args(['--point-rend', '1', '--head-arch', arch]))
        with pytest.raises(ValueError, match='--point-rend 1'):
            evaluate.check_args(evaluate.build_parser().parse_args(['--point-rend', '1', '--head-arch', arch]))
        with pytest.raises(ValueError, match='--point-rend 1'):
            demo.check_args(demo.build_parser().parse_args(['--synthetic', '1', '--point-rend', '1', '--head-arch', arch]))
    with pytest.raises(ValueError, match='--point-rend'):              # train_keypoints.py refuses the flag
        train.run(train.build_parser(keypoints=True).parse_args(['--point-rend', '1']), keypoints=True)
    with pytest.raises(ValueError, match='--point-rend 1.*mask_iou'):
        train.run(train.build_parser().parse_args(['--point-rend', '1', '--mask-iou', '1']))
    with pytest.raises(ValueError, match='--point-rend 1.*mask_iou'):
        evaluate.check_args(evaluate.build_parser().parse_args(['--point-rend', '1', '--mask-iou', '1']))
    with pytest.raises(ValueError, match='--point-rend 1 .*tta'):
        evaluate.check_args(evaluate.build_parser().parse_args(['--point-rend', '1', '--tta-hflip', '1']))
    with pytest.raises(ValueError, match='--point-rend 1 .*tta'):
        demo.check_args(demo.build_parser().parse_args(['--synthetic', '1', '--point-rend', '1', '--tta-sizes', '160', '200']))
    with pytest.raises(ValueError, match='--point-rend 1 .*eval-tta'):
        train.run(train.build_parser().parse_args(['--point-rend', '1', '--eval-tta-hflip', '1']))
    with pytest.raises(ValueError, match='belongs to --point-rend 1'):
        train.run(train.build_parser().parse_args(['--point-loss-weight', '2']))


def test_resume_with_another_setting_is_refused(tmp_path):
    import train
    p = train.build_parser()
    on, off = p.parse_args(['--point-rend', '1']), p.parse_args([])
    fewer, half = p.parse_args(['--point-rend', '1', '--point-train-points', '98']), p.parse_args(['--point-rend', '1', '--point-loss-weight', '0.5'])
    from chainer_maskrcnn.inference_options import EXTENSIONS, check_resume, extension_settings
    e = {x.name: x for x in EXTENSIONS}['point_rend']

    def run_settings(args):
        return extension_settings(args, '--eval-tta-', training=True)['point_rend']

    def check(resume, args, path=''):
        check_resume(resume, e.state_key, e.off, run_settings(args), e.settings_noun, path)
    state = {'point_rend': run_settings(on)}
    assert state['point_rend']['point_rend'] is True and state['point_rend']['point_train_points'] == 196
    ck = str(tmp_path / 'trainer_5.pt')
    torch.save(dict(state, iteration=5), ck)
    state = torch.load(ck, map_location='cpu', weights_only=False)
    check(state, on, ck)
    check({}, off)                                    # a state from before the key existed: no point head
    for resume, args in ((state, off), ({}, on), (state, fewer), (state, half)):
        with pytest.raises(ValueError, match='--resume .* PointRend'):
            check(resume, args, ck)
    old = str(tmp_path / 'trainer_old.pt')
    torch.save({'iteration': 3}, old)
    with pytest.raises(ValueError, match='--resume .* PointRend'):          # through run(): refused before any device work
        train.run(p.parse_args(['--resume', old, '--point-rend', '1']))
    with pytest.raises(ValueError, match='--resume .* PointRend'):
        train.run(p.parse_args(['--resume', ck]))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
NEW = {'mrcnn_point_train_coords': 14, 'mrcnn_point_features_fwd': 17, 'mrcnn_point_features_bwd': 13, 'mrcnn_point_concat_fwd': 10,
       'mrcnn_point_concat_bwd': 6, 'mrcnn_point_target': 16, 'mrcnn_point_bce': 14, 'mrcnn_point_subdivide': 11, 'mrcnn_point_scatter': 10}


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
    hip = open(os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc', 'pointrend.hip')).read()
    assert sorted(re.findall(r'extern "C" (?:int|size_t) (mrcnn_point_\w+)', hip)) == sorted(NEW)
    assert '#include "point_common.h"' in hip and 'asm(' not in hip and 'asm volatile' not in hip and 'atomicAdd(&hist' in hip
    assert hip.count('atomicAdd') == 1 and 'atomicCAS' not in hip and 'atomicExch' not in hip         # the one integer LDS histogram; no float atomic


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _hip.lib()
    A = ctypes.c_void_p(8192)               # an address that is compared, never dereferenced
    f = ctypes.c_float

    def coords(keys=A, nk=1274, coarse=A, S0=28, Cp=96, nch=80, lab=A, base=1, rows=4, P=196, nc=588, ni=147, out=A):
        return lib.mrcnn_point_train_coords(keys, nk, coarse, S0, Cp, nch, lab, base, rows, P, nc, ni, out, None)
    for kw in (dict(keys=None), dict(coarse=None), dict(lab=None), dict(out=None), dict(rows=-1), dict(S0=0), dict(Cp=0), dict(P=0), dict(nc=0),
               dict(ni=-1), dict(ni=197), dict(ni=148, nc=147), dict(nk=1273), dict(nch=0), dict(nch=97)):
        assert coords(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert coords(nc=4097, nk=10000) != 0 and b'candidates' in lib.mrcnn_last_error()
    assert coords(rows=0) == 0 and coords(rows=0, keys=None, out=None) == 0

    def fwd(co=A, roi=A, fmap=A, N=2, H=32, W=40, C=256, sc=0.25, coarse=A, S0=28, Cp=96, nch=80, rows=4, P=196, cin_p=352, out=A):
        return lib.mrcnn_point_features_fwd(co, roi, fmap, N, H, W, C, f(sc), coarse, S0, Cp, nch, rows, P, cin_p, out, None)
    for kw in (dict(co=None), dict(roi=None), dict(fmap=None), dict(coarse=None), dict(out=None), dict(rows=-1), dict(N=0), dict(H=0), dict(W=0),
               dict(C=0), dict(C=254), dict(sc=0.0), dict(sc=float('nan')), dict(S0=0), dict(Cp=0), dict(Cp=98), dict(P=0), dict(cin_p=350),
               dict(cin_p=332), dict(nch=0), dict(nch=97)):
        assert fwd(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert fwd(rows=0) == 0 and fwd(rows=0, co=None) == 0

    def bwd(g=A, ld=352, co=A, roi=A, rows=4, P=196, sc=0.25, gm=A, N=2, H=32, W=40, C=256):
        return lib.mrcnn_point_features_bwd(g, ld, co, roi, rows, P, f(sc), gm, N, H, W, C, None)
    for kw in (dict(g=None), dict(co=None), dict(roi=None), dict(gm=None), dict(rows=-1), dict(P=0), dict(ld=0), dict(ld=254), dict(ld=128),
               dict(sc=-1.0), dict(N=0), dict(H=0), dict(W=0), dict(C=0), dict(C=250)):
        assert bwd(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert bwd(C=1024, ld=1024) != 0 and b'channels' in lib.mrcnn_last_error()
    assert bwd(rows=0) == 0 and bwd(rows=0, g=None) == 0

    def cat(h=A, Ch=256, x0=A, ld0=352, c0=256, nco=80, n=10, cin_p=352, out=A):
        return lib.mrcnn_point_concat_fwd(h, Ch, x0, ld0, c0, nco, n, cin_p, out, None)
    for kw in (dict(h=None), dict(x0=None), dict(out=None), dict(n=-1), dict(Ch=0), dict(Ch=254), dict(ld0=0), dict(c0=-4), dict(c0=258), dict(nco=0),
               dict(cin_p=0), dict(cin_p=332), dict(nco=100), dict(c0=300)):
        assert cat(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert cat(n=0) == 0 and cat(n=0, h=None) == 0

    def uncat(g=A, cin_p=352, Ch=256, n=10, out=A):
        return lib.mrcnn_point_concat_bwd(g, cin_p, Ch, n, out, None)
    for kw in (dict(g=None), dict(out=None), dict(n=-1), dict(Ch=0), dict(Ch=254), dict(cin_p=0), dict(cin_p=128)):
        assert uncat(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert uncat(n=0) == 0

    def target(masks=A, N=2, G=4, H=37, W=45, n_gt=A, roi=A, asg=A, lab=A, n_pos=A, S=12, rows=12, co=A, P=9, out=A):
        return lib.mrcnn_point_target(masks, N, G, H, W, n_gt, roi, asg, lab, n_pos, S, rows, co, P, out, None)
    for kw in (dict(masks=None), dict(n_gt=None), dict(roi=None), dict(asg=None), dict(lab=None), dict(n_pos=None), dict(co=None), dict(out=None),
               dict(N=0), dict(G=0), dict(H=0), dict(W=-1), dict(S=0), dict(rows=-1), dict(rows=13), dict(P=0)):
        assert target(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert target(rows=0) == 0 and target(rows=0, masks=None, out=None) == 0

    def bce(pred=A, ld=96, nch=80, tgt=A, lab=A, base=1, rows=4, P=9, w=1.0, out=A, gx=A, ws=A, wsb=1 << 20):
        return lib.mrcnn_point_bce(pred, ld, nch, tgt, lab, base, rows, P, f(w), out, gx, ws, wsb, None)
    for kw in (dict(pred=None), dict(tgt=None), dict(lab=None), dict(out=None), dict(ws=None), dict(rows=-1), dict(ld=0), dict(P=0), dict(nch=0),
               dict(nch=97), dict(w=0.0), dict(w=-1.0), dict(w=float('nan')), dict(w=float('inf'))):
        assert bce(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert bce(wsb=16) != 0 and b'workspace' in lib.mrcnn_last_error()

    def sub(grid=A, D=3, S=28, ld=96, nch=80, lab=A, n=784, up=A, idx=A, co=A):
        return lib.mrcnn_point_subdivide(grid, D, S, ld, nch, lab, n, up, idx, co, None)
    for kw in (dict(grid=None), dict(up=None), dict(idx=None), dict(co=None), dict(D=-1), dict(S=0), dict(ld=0), dict(n=0), dict(n=3137), dict(nch=0),
               dict(nch=97)):
        assert sub(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert sub(S=57) != 0 and b'56 x 56' in lib.mrcnn_last_error()
    assert sub(D=0) == 0 and sub(D=0, grid=None) == 0

    def scatter(pred=A, ld=96, nch=80, lab=A, idx=A, D=3, n=784, cells=3136, grid=A):
        return lib.mrcnn_point_scatter(pred, ld, nch, lab, idx, D, n, cells, grid, None)
    for kw in (dict(pred=None), dict(idx=None), dict(grid=None), dict(D=-1), dict(ld=0), dict(n=0), dict(cells=0), dict(nch=0), dict(nch=97)):
        assert scatter(**kw) == -1 and lib.mrcnn_last_error(), kw
    assert scatter(D=0) == 0 and scatter(D=0, pred=None) == 0


def test_ops_have_no_cpu_fallback():
    i32 = torch.int32
    z = torch.zeros
    calls = [lambda: ops.point_train_coords(z((1, 20), dtype=i32), z((1, 6, 6, 32)), z((1,), dtype=i32), 3, 4, 8, 3),
             lambda: ops.point_features_fwd(z((1, 4, 2)), z((1, 5)), z((1, 8, 8, 32)), 0.25, z((1, 6, 6, 32)), 3, 64),
             lambda: ops.point_features_bwd(z((1, 1, 4, 64)), z((1, 4, 2)), z((1, 5)), 0.25, z((1, 8, 8, 32))),
             lambda: ops.point_concat_fwd(z((1, 1, 4, 64)), z((1, 1, 4, 64)), 32, 3, 96),
             lambda: ops.point_concat_bwd(z((1, 1, 4, 96)), 64),
             lambda: ops.point_target(z((1, 1, 8, 8), dtype=torch.uint8), torch.ones((1,), dtype=i32), z((2, 5)), z((2,), dtype=i32), z((2,), dtype=i32),
                                      torch.ones((1,), dtype=i32), 2, 2, z((2, 4, 2))),
             lambda: ops.point_bce(z((2, 1, 4, 32)), z((2, 4)), z((2,), dtype=i32), 3),
             lambda: ops.point_subdivide(z((1, 4, 4, 32)), z((1,), dtype=i32), 3, 5),
             lambda: ops.point_scatter(z((1, 1, 5, 32)), z((1,), dtype=i32), z((1, 5), dtype=i32), 3, z((1, 8, 8)))]
    for call in calls:
        with pytest.raises(_hip.MrcnnHipError):
            call()
    assert ops.point_n_keys(196, 588, 147) == 2 * 588 + 2 * 49
