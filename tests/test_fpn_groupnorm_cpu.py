"""CPU tests of GroupNorm in the FPN: the references of tests/fpn_groupnorm_reference.py against torch, the plan
query and the argument checks of the map entry points (no device), the model structure with and without ``fpn_norm``, the NPZ mapping and
the flags of the four scripts."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from chainer_maskrcnn import _hip
from chainer_maskrcnn._hip import ops
from chainer_maskrcnn.model.maskrcnn import MaskRCNN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpn_groupnorm_reference as fgr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SHRINK = dict(stages=(1, 1, 1, 1), width_div=4)
FPN_CONVS = ['toplayer', 'conv_p4', 'conv_p3', 'conv_p2', 'conv_p6', 'lat_p4', 'lat_p3', 'lat_p2']


# ---- the references ----------------------------------------------------------------------------------------------------------------------
def test_float32_reference_is_the_float64_one_within_rounding():
    rs = np.random.RandomState(0)
    x, gy = rs.standard_normal((2, 9, 7, 64)) * 2 + 3, rs.standard_normal((2, 9, 7, 64))
    gamma, beta = rs.standard_normal(64) + 1, rs.standard_normal(64)
    a, b = fgr.all_six(x, gy, gamma, beta, 48, 12, np.float64), fgr.all_six(x, gy, gamma, beta, 48, 12, np.float32)
    for k in a:
        assert b[k].dtype == np.float32 and a[k].dtype == np.float64 and a[k].shape == b[k].shape
        err = np.abs(a[k] - b[k]).max() / max(np.abs(a[k]).max(), 1e-6)
        assert 0 < err < 1e-5, (k, err)
    assert not a['y'][..., 48:].any() and not a['gx'][..., 48:].any() and not a['ggamma'][48:].any()


def test_top_down_reference_has_the_pyramid_shapes():
    g = torch.Generator().manual_seed(0)
    fc, cins = 16, {'toplayer': 64, 'lat_p4': 32, 'lat_p3': 16, 'lat_p2': 8}
    P = {}
    for n in fgr.FPN_CONVS:
        k = 3 if n in ('conv_p4', 'conv_p3', 'conv_p2') else 1
        P[n + '/W'] = torch.randn((fc, k, k, cins.get(n, fc)), generator=g, dtype=torch.float64) * 0.1
        P[n + '/b'] = torch.randn(fc, generator=g, dtype=torch.float64)
        P[n + '/gn/gamma'] = torch.randn(fc, generator=g, dtype=torch.float64)
        P[n + '/gn/beta'] = torch.randn(fc, generator=g, dtype=torch.float64)
    cs = [torch.randn((1, h, w, c), generator=g, dtype=torch.float64) for h, w, c in ((9, 13, 8), (5, 7, 16), (3, 4, 32), (2, 2, 64))]
    shapes = [(1, 9, 13, fc), (1, 5, 7, fc), (1, 3, 4, fc), (1, 2, 2, fc), (1, 1, 1, fc)]
    grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    ps, gcs, gr = fgr.top_down(P, cs, grads, 4, torch.float64)
    assert [tuple(p.shape) for p in ps] == shapes and [tuple(a.shape) for a in gcs] == [tuple(c.shape) for c in cs]
    assert set(gr) == set(P) and all(gr[n].shape == P[n].shape and float(gr[n].abs().max()) > 0 for n in P)


# ---- plan query and argument checks: host arithmetic, no device --------------------------------------------------------------------------
def _plan_rc(R, H, W, C, Cp, G):
    out = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = _hip.lib().mrcnn_group_norm_map_plan(R, H, W, C, Cp, G, *[ctypes.byref(o) for o in out])
    return (rc,) + tuple(o.value for o in out)


@pytest.mark.parametrize('Cp,C,G', [(256, 256, 32), (64, 64, 16), (32, 32, 8), (64, 48, 12), (128, 128, 2)])
def test_plan_covers_the_map_with_its_chunks(Cp, C, G):
    seen = set()
    for hw in list(range(1, 700)) + [1024, 4096, 16384, 65536, 65537, 1 << 20]:
        ppc, chunks, nf, nb = ops.group_norm_map_plan(2, 1, hw, C, Cp, G)
        assert chunks * ppc >= hw > (chunks - 1) * ppc, (hw, ppc, chunks)
        assert nf == (2 * 2 * chunks * G + 2 * 2 * G) * 4 and nb == (2 * 2 * chunks * Cp + 2 * 2 * G) * 4
        assert ops.group_norm_map_plan(2, hw, 1, C, Cp, G) == (ppc, chunks, nf, nb)          # a function of H * W
        seen.add(min(chunks, 3))
    assert seen == {1, 2, 3}


def test_plan_spreads_the_pyramid_levels_and_is_monotone_in_r():
    chunks = {hw: ops.group_norm_map_plan(2, hw, hw, 256, 256, 32)[1] for hw in (256, 128, 64, 32)}
    assert 2 * chunks[256] >= 2 * 256                        # P2: at least two workgroups per CU
    assert 2 * chunks[64] >= 128 and 2 * chunks[32] >= 32    # P4 and P5 do not collapse onto a handful of workgroups
    for shape in ((64, 64, 256, 256, 32), (37, 53, 48, 64, 12)):
        plans = [ops.group_norm_map_plan(R, *shape) for R in range(0, 20)]
        assert plans[0][2:] == (0, 0)                        # R == 0 is valid
        assert len({p[:2] for p in plans}) == 1              # the grid of a sample does not depend on the batch it arrives in
        assert all(a[2] <= b[2] and a[3] <= b[3] for a, b in zip(plans, plans[1:]))


@pytest.mark.parametrize('geom,word', [((2, 40, 40, 64, 64, 64), b'multiple of 4'), ((2, 40, 40, 64, 64, 32), b'multiple of 4'),
                                       ((2, 40, 40, 48, 64, 16), b'multiple of 4'), ((2, 40, 40, 512, 512, 1), b'multiple of 4'),
                                       ((2, 40, 40, 2048, 2048, 32), b'above'), ((2, 40, 40, 64, 64, 24), b'divide'),
                                       ((2, 40, 40, 64, 32, 16), b'below'), ((2, 40, 40, 64, 66, 16), b'multiple of 4'),
                                       ((2, 0, 40, 64, 64, 16), b'H x W'), ((2, 40, -1, 64, 64, 16), b'H x W'), ((2, 40, 40, 0, 64, 16), b'positive'),
                                       ((2, 40, 40, 64, 64, 0), b'positive'), ((-1, 40, 40, 64, 64, 16), b'negative'),
                                       ((2, 65536, 512, 64, 64, 16), b'int32')])
def test_plan_refuses_what_the_map_path_does_not_take(geom, word):
    """cpg 1, 2 and 3 (and one above 256, and Cp above 1024) belong to group_norm_*; the rest is invalid everywhere."""
    rc, ppc, chunks, nf, nb = _plan_rc(*geom)
    assert rc == -1 and (ppc, chunks, nf, nb) == (-7, -7, 0, 0)
    assert word in _hip.lib().mrcnn_last_error(), _hip.lib().mrcnn_last_error()
    with pytest.raises(_hip.MrcnnHipError):
        ops.group_norm_map_plan(*geom)


def test_compute_entry_points_refuse_bad_arguments_without_a_device():
    lib = _hip.lib()
    A, ODD = ctypes.c_void_p(8192), ctypes.c_void_p(8196)         # addresses that are compared, never dereferenced
    GOOD = (2, 40, 40, 64, 64, 16)
    _, _, nf, nb = ops.group_norm_map_plan(*GOOD)

    def fwd(q=None, geom=GOOD, eps=1e-5, ws_bytes=nf):
        p = [A] * 5
        for k, v in (q or {}).items():
            p[k] = v
        x, gamma, beta, y, ws = p
        return lib.mrcnn_group_norm_map_fwd_f32(x, gamma, beta, *geom, eps, y, None, None, ws, ws_bytes, None)

    def bwd(q=None, geom=GOOD, ws_bytes=nb):
        p = [A] * 9
        for k, v in (q or {}).items():
            p[k] = v
        gy, x, gamma, mean, rstd, gx, gg, gb, ws = p
        return lib.mrcnn_group_norm_map_bwd_f32(gy, x, gamma, mean, rstd, *geom, gx, gg, gb, 0, ws, ws_bytes, None)

    for k in range(5):
        assert fwd({k: None}) == -1 and lib.mrcnn_last_error(), k
        assert fwd({k: ODD}) == -1 and b'aligned' in lib.mrcnn_last_error(), k
    for k in range(9):
        assert bwd({k: None}) == -1 and lib.mrcnn_last_error(), k
    for k in (0, 1, 2, 5, 6, 7, 8):
        assert bwd({k: ODD}) == -1 and b'aligned' in lib.mrcnn_last_error(), k
    assert fwd(eps=0.0) == -1 and fwd(eps=-1.0) == -1
    assert fwd(ws_bytes=nf - 1) == -1 and b'workspace' in lib.mrcnn_last_error() and fwd(ws_bytes=0) == -1
    assert bwd(ws_bytes=nb - 1) == -1 and b'workspace' in lib.mrcnn_last_error() and bwd(ws_bytes=0) == -1
    for geom in ((2, 40, 40, 64, 64, 24), (2, 40, 40, 64, 32, 16), (2, 40, 40, 64, 66, 16), (2, 40, 0, 64, 64, 16), (2, -3, 40, 64, 64, 16),
                 (2, 40, 40, 0, 64, 16), (2, 40, 40, 64, 64, -1), (-2, 40, 40, 64, 64, 16), (2, 65536, 512, 64, 64, 16),
                 (2, 40, 40, 64, 64, 64), (2, 40, 40, 64, 64, 32), (2, 40, 40, 48, 64, 16)):
        assert fwd(geom=geom, ws_bytes=1 << 40) == -1 and bwd(geom=geom, ws_bytes=1 << 40) == -1, geom
    # R == 0 succeeds without a launch
    assert fwd(geom=(0,) + GOOD[1:], ws_bytes=0) == 0 and bwd(geom=(0,) + GOOD[1:], ws_bytes=0) == 0


def test_ops_have_no_cpu_fallback():
    x = torch.zeros((2, 40, 40, 64))
    g, b = torch.ones(64), torch.zeros(64)
    with pytest.raises(_hip.MrcnnHipError):
        ops.group_norm_map_fwd(x, g, b, 64, 16)
    with pytest.raises(_hip.MrcnnHipError):
        ops.group_norm_map_bwd(x, x, g, torch.zeros((2, 16)), torch.ones((2, 16)), 64, 16)


def test_map_argument_checks_under_host_sanitizers(tmp_path):
    """The same checks and the plan query, swept wider, in a stand-alone program (tests/native/groupnorm_map_host_check.cpp, its own main)
    built together with groupnorm_map.hip and lib.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code (the device
    code is compiled as usual) and run on the CPU: every compute call is refused before a launch, so no device is touched."""
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    csrc = os.path.join(ROOT, 'chainer-maskrcnn_amd', 'csrc')
    exe = str(tmp_path / 'groupnorm_map_host_check')
    subprocess.check_call([hipcc, '-std=c++17', '-O1', '-g', '--offload-arch=gfx950', '-ffp-contract=off', '-Xarch_host',
                           '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined', '-I' + os.path.join(ROOT, 'include'),
                           '-I' + csrc, os.path.join(csrc, 'groupnorm_map.hip'), os.path.join(csrc, 'lib.hip'), '-x', 'c++',
                           os.path.join(ROOT, 'tests', 'native', 'groupnorm_map_host_check.cpp'), '-o', exe], cwd=str(tmp_path))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and b'groupnorm_map_host_check: ok' in r.stdout, r.stdout.decode('utf-8', 'replace')[-2000:]


def test_layer_picks_its_kernels_from_the_shape():
    from chainer_maskrcnn.nn.core import GroupNorm, MapGroupNorm, ParamStore
    ps = ParamStore()
    a, b, c = MapGroupNorm(ps, 'a/gn', 64, 16), MapGroupNorm(ps, 'b/gn', 64, 32), MapGroupNorm(ps, 'c/gn', 256, 32)
    assert isinstance(a, GroupNorm) and list(ps.offsets) == ['a/gn/gamma', 'a/gn/beta', 'b/gn/gamma', 'b/gn/beta', 'c/gn/gamma', 'c/gn/beta']
    assert not a.uses_map_path((2, 16, 16, 64))              # the register path where it reaches
    assert a.uses_map_path((2, 37, 53, 64))
    assert not b.uses_map_path((2, 33, 31, 64))              # cpg 2: generic
    assert not c.uses_map_path((2, 14, 14, 256)) and c.uses_map_path((2, 32, 32, 256)) and c.uses_map_path((2, 256, 256, 256))
    with pytest.raises(ValueError):
        MapGroupNorm(ps, 'd/gn', 64, 24)


# ---- model structure ---------------------------------------------------------------------------------------------------------------------
def _model(seed=1, keypoints=False, **kw):
    if keypoints:
        return MaskRCNN(n_fg_class=1, n_keypoints=17, head_arch='fpn_keypoint', device='cpu', seed=seed, _test_shrink=SHRINK, **kw)
    return MaskRCNN(n_fg_class=5, device='cpu', seed=seed, _test_shrink=SHRINK, **kw)


@pytest.mark.parametrize('keypoints', [False, True], ids=['mask', 'keypoint'])
def test_fpn_norm_adds_only_its_own_parameters(keypoints):
    plain, off, gn = _model(keypoints=keypoints), _model(keypoints=keypoints, fpn_norm=None), _model(keypoints=keypoints, fpn_norm='gn', gn_groups=16)
    assert off.ps.offsets == plain.ps.offsets and off.ps.size == plain.ps.size
    assert not any('/gn/' in n for n in off.ps.offsets)
    assert torch.equal(off.ps.params, plain.ps.params)
    want = ['extractor/%s/gn/%s' % (c, k) for c in FPN_CONVS for k in ('gamma', 'beta')]
    added = [n for n in gn.ps.offsets if n not in plain.ps.offsets]
    assert added == want and len(added) == 16                # in registration order
    assert [n for n in gn.ps.offsets if n in plain.ps.offsets] == list(plain.ps.offsets)
    names = list(gn.ps.offsets)
    fc = gn.extractor.out_channels
    assert fc == 64
    for c in FPN_CONVS:                  # registered directly behind their convolution
        i = names.index('extractor/%s/b' % c)
        assert names[i + 1:i + 3] == ['extractor/%s/gn/gamma' % c, 'extractor/%s/gn/beta' % c]
        assert gn.ps.offsets['extractor/%s/gn/gamma' % c][1] == (fc,) and gn.ps.offsets['extractor/%s/gn/beta' % c][1] == (fc,)
        g, b = gn.ps.p('extractor/%s/gn/gamma' % c), gn.ps.p('extractor/%s/gn/beta' % c)
        assert torch.equal(g, torch.ones(fc)) and not b.any()
        layer = gn.extractor.norms['extractor/' + c]
        assert layer.groups == 16 and layer.c == fc
    for n in plain.ps.offsets:           # every other name keeps its shape and its initial value
        assert gn.ps.offsets[n][1] == plain.ps.offsets[n][1] and torch.equal(gn.ps.p(n), plain.ps.p(n)), n
    # the FPN's parameters still start at toplayer and the RPN's follow them
    assert min(o for n, (o, _) in gn.ps.offsets.items() if '/gn/' in n) > gn.ps.offsets['extractor/toplayer/W'][0]
    assert max(o for n, (o, _) in gn.ps.offsets.items() if '/gn/' in n) < min(o for n, (o, _) in gn.ps.offsets.items() if n.startswith('rpn/'))
    assert plain.extractor.norms == {} and plain.extractor.fpn_norm is None and gn.extractor.fpn_norm == 'gn'


def test_padded_gamma_is_one_on_the_logical_channels_only():
    from chainer_maskrcnn.model.extractor.feature_pyramid_network import FeaturePyramidNetwork
    fpn = FeaturePyramidNetwork(stages=(1, 1, 1, 1), width_div=16, fpn_norm='gn', gn_groups=4)       # 16 channels padded to 32
    fpn.ps.materialise(torch.device('cpu'), 1)
    for c in FPN_CONVS:
        g, b = fpn.ps.p('extractor/%s/gn/gamma' % c), fpn.ps.p('extractor/%s/gn/beta' % c)
        assert g.shape == (32,) and torch.equal(g[:16], torch.ones(16)) and not g[16:].any() and not b.any()


def test_two_seeds_differ_only_where_they_did_before():
    p1, p2, g1, g2 = _model(1), _model(2), _model(1, fpn_norm='gn'), _model(2, fpn_norm='gn')
    for n in p1.ps.offsets:
        assert torch.equal(p1.ps.p(n), p2.ps.p(n)) == torch.equal(g1.ps.p(n), g2.ps.p(n)), n
        assert torch.equal(p2.ps.p(n), g2.ps.p(n)), n
    for n in g1.ps.offsets:
        if '/gn/' in n:
            assert torch.equal(g1.ps.p(n), g2.ps.p(n))


def test_fpn_norm_is_refused_where_it_does_not_exist():
    with pytest.raises(ValueError, match='fpn_norm'):
        MaskRCNN(n_fg_class=5, backbone='c4', head_arch='res5', device='cpu', _test_shrink=dict(width_div=4), fpn_norm='gn')
    with pytest.raises(ValueError, match='fpn_norm'):
        MaskRCNN(n_fg_class=5, backbone='darknet', device='cpu', fpn_norm='gn')
    with pytest.raises(ValueError, match='fpn_norm'):
        _model(fpn_norm='bn')
    with pytest.raises(ValueError, match='gn_groups'):
        _model(fpn_norm='gn', gn_groups=48)              # 64 channels under the shrink
    _model(gn_groups=48)                                 # ignored without a norm
    both = _model(fpn_norm='gn', head_norm='gn', gn_groups=16)
    assert both.head.gn1.groups == 16 and both.extractor.norms['extractor/lat_p2'].groups == 16
    assert sum('/gn/' in n for n in both.ps.offsets) == 16 + 10


def test_freezing_leaves_the_fpn_norm_trainable():
    m = _model(fpn_norm='gn')
    for at in (0, 2, 5):
        frozen = m.extractor.set_freeze(bn=True, at=at)
        assert not any('/gn/' in n for n in frozen)


# ---- NPZ ----------------------------------------------------------------------------------------------------------------------------------
def test_npz_round_trip_with_fpn_group_norm(tmp_path):
    from chainer_maskrcnn.utils.chainer_npz import ChainerNpzMap, load_npz, save_npz
    a, b = _model(1, fpn_norm='gn', head_norm='gn'), _model(2, fpn_norm='gn', head_norm='gn')
    rs = np.random.RandomState(3)
    c = a.extractor.out_channels
    gns = [n for n in a.ps.offsets if n.startswith('extractor/') and '/gn/' in n]
    assert len(gns) == 16
    for n in gns:
        a.ps.p(n)[:c] = torch.from_numpy(rs.standard_normal(c).astype(np.float32))
    d = ChainerNpzMap(a).to_chainer()
    assert all(d[n].shape == (c,) for n in gns)          # logical channels only
    path = str(tmp_path / 'gn.npz')
    save_npz(path, a)
    loaded = load_npz(path, b, strict=True)
    assert set(gns) <= set(loaded)
    assert torch.equal(a.ps.params, b.ps.params)
    # a plain snapshot loads into a GroupNorm model and leaves gamma = 1, beta = 0
    plain, fresh = _model(4), _model(6, fpn_norm='gn')
    path2 = str(tmp_path / 'plain.npz')
    save_npz(path2, plain)
    loaded = load_npz(path2, fresh)
    assert not any('/gn/' in k for k in loaded)
    assert all(torch.equal(fresh.ps.p(n), torch.ones(c) if n.endswith('gamma') else torch.zeros(c)) for n in gns)
    for n in plain.ps.offsets:
        assert torch.equal(plain.ps.p(n), fresh.ps.p(n)), n
    with pytest.raises(KeyError):
        load_npz(path2, fresh, strict=True)


# ---- flags --------------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_in_all_four_scripts():
    import demo
    import evaluate
    import train
    for parser in (train.build_parser(), train.build_parser(keypoints=True), evaluate.build_parser(), demo.build_parser()):
        a = parser.parse_args([])
        assert a.fpn_norm == 'none' and a.head_norm == 'none' and a.gn_groups == 32
        a = parser.parse_args(['--fpn-norm', 'gn', '--gn-groups', '16'])
        assert a.fpn_norm == 'gn' and a.head_norm == 'none' and a.gn_groups == 16
        with pytest.raises(SystemExit):
            parser.parse_args(['--fpn-norm', 'bn'])
    a = train.build_parser(keypoints=True).parse_args(['--fpn_norm', 'gn'])       # train_keypoints.py takes both spellings
    assert a.fpn_norm == 'gn'
    from chainer_maskrcnn.inference_options import fpn_norm_settings, head_norm_settings
    assert fpn_norm_settings('none', 32, 'fpn') == {'fpn_norm': None} and fpn_norm_settings('gn', 16, 'fpn') == {'fpn_norm': 'gn'}
    assert fpn_norm_settings('none', 48, 'c4') == {'fpn_norm': None}
    assert head_norm_settings('gn', 16, 'fpn') == {'head_norm': 'gn', 'gn_groups': 16}           # as it was


@pytest.mark.parametrize('backbone,arch', [('c4', 'res5'), ('darknet', 'fpn')])
def test_flag_is_refused_off_the_fpn(backbone, arch):
    import demo
    import evaluate
    import train
    from chainer_maskrcnn.inference_options import fpn_norm_settings
    with pytest.raises(ValueError, match='--fpn-norm gn'):
        fpn_norm_settings('gn', 32, backbone)
    flags = ['--fpn-norm', 'gn', '--backbone', backbone, '--head-arch', arch]
    with pytest.raises(ValueError, match='--fpn-norm gn'):
        train.run(train.build_parser().parse_args(flags))
    with pytest.raises(ValueError, match='--fpn-norm gn'):
        evaluate.check_args(evaluate.build_parser().parse_args(flags))
    with pytest.raises(ValueError, match='--fpn-norm gn'):
        demo.check_args(demo.build_parser().parse_args(['--synthetic', '1'] + flags))
    with pytest.raises(ValueError, match='--gn-groups'):
        fpn_norm_settings('gn', 48, 'fpn')
    with pytest.raises(ValueError, match='--fpn-norm'):
        fpn_norm_settings('bn', 32, 'fpn')
