"""CPU tests of test-time augmentation (MaskRCNN.use_test_augmentation, csrc/tta.hip): the view list, the refused settings, the argument
errors of the new C entry points (reported before any device work) and the TTA flags of evaluate.py / train.py."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn import _hip  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402


def _model(head_arch='fpn', K=17, min_size=600, max_size=1000):
    m = MaskRCNN.__new__(MaskRCNN)          # the TTA settings read only these attributes
    m.head_arch, m.min_size, m.max_size, m.tta = head_arch, min_size, max_size, None
    m.head = types.SimpleNamespace(n_keypoints=K)
    return m


def test_views_order_sizes_and_max_size():
    m = _model()
    assert m.tta is None
    m.use_test_augmentation([800, 600], hflip=True)
    assert m.test_views(480, 640) == [(750, 1000, False), (750, 1000, True), (600, 800, False), (600, 800, True)]
    assert m.test_views(640, 427) == [(1000, 667, False), (1000, 667, True), (899, 600, False), (899, 600, True)]
    m.use_test_augmentation([500], max_size=600)
    assert m.test_views(480, 640) == [(450, 600, False)]
    m.use_test_augmentation([600])
    assert m.test_views(480, 640) == [m.prepare_size(480, 640) + (False,)]    # one unmirrored view at min_size = prepare()
    m.use_test_augmentation(None)
    assert m.tta is None


def test_views_follow_prepare_size_rule():
    from chainer_maskrcnn.model.maskrcnn import scaled_size
    m = _model(min_size=512, max_size=700)
    rs = np.random.RandomState(0)
    for _ in range(50):
        H, W = (int(v) for v in rs.randint(1, 1500, 2))
        s, ms = int(rs.randint(1, 1200)), int(rs.randint(1, 1600))
        m.use_test_augmentation([s], max_size=ms)
        scale = s / min(H, W)
        if scale * max(H, W) > ms:
            scale = ms / max(H, W)
        assert m.test_views(H, W) == [(int(H * scale), int(W * scale), False)] == [scaled_size(H, W, s, ms) + (False,)]
        assert m.prepare_size(H, W) == scaled_size(H, W, 512, 700)


def test_refused_settings():
    m = _model()
    for bad in ([600, 600], [0], [-5, 600], []):
        with pytest.raises(ValueError):
            m.use_test_augmentation(bad)
    with pytest.raises(ValueError):
        m.use_test_augmentation([1, 2, 3, 4, 5], hflip=True)        # 10 views > 8
    m.use_test_augmentation([1, 2, 3, 4], hflip=True)                # 8 views
    assert len(m.test_views(100, 100)) == 8
    with pytest.raises(ValueError):
        m.use_test_augmentation([600], max_size=0)
    kp = _model('fpn_keypoint', K=17)
    with pytest.raises(ValueError, match='keypoint_flip_perm'):
        kp.use_test_augmentation([600], hflip=True)
    with pytest.raises(ValueError):
        kp.use_test_augmentation([600], hflip=True, keypoint_flip_perm=[0] * 17)
    from chainer_maskrcnn.dataset import augment
    kp.use_test_augmentation([600], hflip=True, keypoint_flip_perm=augment.flip_permutation(augment.COCO_KEYPOINT_NAMES))
    kp.use_test_augmentation([600, 800])                             # no mirror: no flip map needed
    assert kp.tta['keypoint_flip_perm'] is None


# ---- argument errors of the C entry points (no device: every call must fail before a launch) --------------------------------------------
_BUF = (ctypes.c_float * 4096)()
A = ctypes.addressof(_BUF)            # a host address used as an opaque "device pointer" that is never dereferenced


def _views(rows):
    return ops.tta_views(rows)


def _err(rc, code=-1):
    assert rc == code, (rc, _hip.lib().mrcnn_last_error())


def test_resize_mirror_argument_errors():
    lib = _hip.lib()
    _err(lib.mrcnn_image_resize_mirror_f32(None, 3, 4, 4, A, 4, 4, 4, 4, 0, 1.0, None))
    _err(lib.mrcnn_image_resize_mirror_f32(A, 3, 4, 4, A, 4, 4, 4, 4, 2, 1.0, None))
    _err(lib.mrcnn_image_resize_mirror_f32(A, 3, 0, 4, A, 4, 4, 4, 4, 0, 1.0, None))
    _err(lib.mrcnn_image_resize_mirror_f32(A, 3, 4, 4, A, 4, 5, 4, 4, 1, 1.0, None))
    assert b'mirror' in lib.mrcnn_last_error() or b'sizes' in lib.mrcnn_last_error()


def test_decode_argument_errors():
    lib = _hip.lib()
    ptrs = (ctypes.c_void_p * 2)(A, A)
    m4 = (ctypes.c_float * 4)()
    good = _views([(3, 0, 1.5), (2, 1, 0.5)])
    call = lambda v, V, ld=96, nc=81, loc0=88, h=480.0, w=640.0, p=ptrs: lib.mrcnn_tta_detect_decode_f32(
        ctypes.cast(p, ctypes.c_void_p), ctypes.cast(p, ctypes.c_void_p), v.ctypes.data, V, ld, nc, loc0, ctypes.cast(m4, ctypes.c_void_p),
        ctypes.cast(m4, ctypes.c_void_p), h, w, A, A, None)
    _err(call(good, 0))
    _err(call(good, 9))
    _err(call(_views([(3, 2, 1.5)]), 1))                 # mirror outside 0 / 1
    _err(call(_views([(3, 0, 0.0)]), 1))                 # scale <= 0
    _err(call(_views([(-1, 0, 1.0)]), 1))                # negative R
    _err(call(good, 2, ld=90))                           # ld < loc0 + 4
    _err(call(good, 2, w=0.0))
    nul = (ctypes.c_void_p * 2)(A, None)
    _err(call(good, 2, p=nul))                           # a view with candidates and no pointer
    assert lib.mrcnn_tta_detect_decode_f32(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(ptrs, ctypes.c_void_p), None, 1, 96, 81, 88,
                                           ctypes.cast(m4, ctypes.c_void_p), ctypes.cast(m4, ctypes.c_void_p), 1.0, 1.0, A, A, None) == -1


def test_class_nms_ws_argument_errors_and_workspace():
    lib = _hip.lib()
    assert lib.mrcnn_class_nms_workspace_bytes(512, 81) == 0          # the LDS kernel needs none
    n600, n4096 = lib.mrcnn_class_nms_workspace_bytes(600, 81), lib.mrcnn_class_nms_workspace_bytes(4096, 81)
    assert n600 >= 81 * 600 * (16 + 4 + 10 * 8) and n4096 >= 81 * 4096 * (16 + 4 + 64 * 8) and n600 % 256 == 0
    assert lib.mrcnn_class_nms_workspace_bytes(4097, 81) == 0
    ws = (ctypes.c_uint8 * 1024)()
    base = (ctypes.addressof(ws) + 255) & ~255
    call = lambda R, ws_ptr, nb, nc=81, lb=1, le=80: lib.mrcnn_class_nms_ws_f32(A, A, R, nc, lb, le, 0.05, 0.3, A, A, ws_ptr, nb, None)
    _err(call(4097, base, n4096), -2)                                  # R > 4096: unsupported
    _err(call(600, base, n600 - 1), -3)                                # short workspace
    _err(call(600, None, n600), -3)                                    # no workspace
    _err(call(600, base + 8, n600), -1)                                # misaligned workspace
    assert b'aligned' in lib.mrcnn_last_error()
    _err(call(0, base, n600))
    _err(call(600, base, n600, le=82))                                 # l_end > n_class
    _err(call(600, base, n600, lb=5, le=4))
    _err(lib.mrcnn_class_nms_ws_f32(None, A, 600, 81, 1, 80, 0.05, 0.3, A, A, base, n600, None))


def test_merge_and_paste_argument_errors():
    lib = _hip.lib()
    ptrs = (ctypes.c_void_p * 3)(A, A, A)
    p = ctypes.cast(ptrs, ctypes.c_void_p)
    v3 = _views([(0, 0, 1.0), (0, 1, 1.0), (0, 0, 1.0)])
    _err(lib.mrcnn_tta_mask_merge_f32(p, v3.ctypes.data, 0, 5, 28, 96, A, A, None))
    _err(lib.mrcnn_tta_mask_merge_f32(p, v3.ctypes.data, 9, 5, 28, 96, A, A, None))
    _err(lib.mrcnn_tta_mask_merge_f32(p, _views([(0, 3, 1.0)]).ctypes.data, 1, 5, 28, 96, A, A, None))
    _err(lib.mrcnn_tta_mask_merge_f32(p, v3.ctypes.data, 3, -1, 28, 96, A, A, None))
    _err(lib.mrcnn_tta_mask_merge_f32(p, v3.ctypes.data, 3, 5, 0, 96, A, A, None))
    _err(lib.mrcnn_tta_mask_merge_f32(p, v3.ctypes.data, 3, 5, 28, 96, None, A, None))
    _err(lib.mrcnn_tta_mask_merge_f32(ctypes.cast((ctypes.c_void_p * 3)(A, None, A), ctypes.c_void_p), v3.ctypes.data, 3, 5, 28, 96, A, A,
                                      None))
    assert lib.mrcnn_tta_mask_merge_f32(p, v3.ctypes.data, 3, 0, 28, 96, None, None, None) == 0       # D == 0: nothing to do
    al = (A + 15) & ~15
    _err(lib.mrcnn_mask_paste_prob_f32(A, 2, 28, al, 0, 10, A, None))
    _err(lib.mrcnn_mask_paste_prob_f32(None, 2, 28, al, 10, 10, A, None))
    _err(lib.mrcnn_mask_paste_prob_f32(A, 2, 28, al + 4, 10, 10, A, None))                            # misaligned boxes
    assert lib.mrcnn_mask_paste_prob_f32(None, 0, 28, None, 10, 10, None, None) == 0


def test_keypoint_merge_argument_errors():
    lib = _hip.lib()
    ptrs = (ctypes.c_void_p * 2)(A, A)
    p = ctypes.cast(ptrs, ctypes.c_void_p)
    v2 = _views([(0, 0, 1.0), (0, 1, 1.0)])
    perm = np.array([0, 2, 1], np.int32)
    call = lambda v, V, K=3, Cp=32, pm=perm, D=4: lib.mrcnn_tta_keypoint_merge_f32(p, v.ctypes.data, V, D, 56, Cp, K,
                                                                                    pm.ctypes.data if pm is not None else None, A, None)
    _err(call(v2, 0))
    _err(call(v2, 9))
    _err(call(v2, 2, pm=None))                                          # a mirrored view without the flip map
    _err(call(v2, 2, pm=np.array([0, 1, 1], np.int32)))                 # not a permutation
    _err(call(v2, 2, pm=np.array([0, 1, 3], np.int32)))
    _err(call(v2, 2, K=33))                                             # Cp < K
    _err(call(v2, 2, K=300, Cp=320, pm=np.arange(300, dtype=np.int32)), -2)
    _err(call(v2, 2, D=-1))
    assert b'keypoint_merge' in lib.mrcnn_last_error()


# ---- flags ----------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_flags():
    import evaluate
    from train import tta_settings
    a = evaluate.build_parser().parse_args([])
    assert a.tta_sizes is None and a.tta_hflip == 0 and a.tta_max_size is None
    assert tta_settings(a.tta_sizes, a.tta_hflip, a.tta_max_size, 600) is None
    a = evaluate.build_parser().parse_args(['--tta-hflip', '1'])
    assert tta_settings(a.tta_sizes, a.tta_hflip, a.tta_max_size, 600) == {'sizes': [600], 'hflip': True, 'max_size': None}
    a = evaluate.build_parser().parse_args(['--tta-sizes', '640', '800', '1000', '--tta-hflip', '1', '--tta-max-size', '1333'])
    assert tta_settings(a.tta_sizes, a.tta_hflip, a.tta_max_size, 600) == {'sizes': [640, 800, 1000], 'hflip': True, 'max_size': 1333}
    a = evaluate.build_parser().parse_args(['--tta-sizes', '700'])
    assert tta_settings(a.tta_sizes, a.tta_hflip, a.tta_max_size, 600) == {'sizes': [700], 'hflip': False, 'max_size': None}
    with pytest.raises(ValueError):
        tta_settings(None, 0, 1333, 600)
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(['--tta-hflip', '2'])


def test_train_flags():
    import train
    from train import tta_settings
    for keypoints in (False, True):
        a = train.build_parser(keypoints=keypoints).parse_args([])
        assert a.eval_tta_sizes is None and a.eval_tta_hflip == 0 and a.eval_tta_max_size is None
        a = train.build_parser(keypoints=keypoints).parse_args(['--eval-tta-sizes', '500', '700', '--eval-tta-hflip', '1',
                                                                '--eval-tta-max-size', '900'])
        assert tta_settings(a.eval_tta_sizes, a.eval_tta_hflip, a.eval_tta_max_size, 600) == {'sizes': [500, 700], 'hflip': True,
                                                                                               'max_size': 900}
