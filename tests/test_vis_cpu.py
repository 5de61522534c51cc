"""CPU tests of the rendering of detections (csrc/vis.hip, chainer_maskrcnn/vis.py, demo.py): the contract's integer rules on hand-made
cases through the NumPy restatement tests/vis_reference.py (the GPU tests hold the kernel to the same restatement bit for bit), the host
half of draw_instances / draw_keypoints (palette, font, label text, drawing order, primitive array), demo.py's flags and refusals, and
the entry point's argument errors, which need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import vis_reference as ref  # noqa: E402
from chainer_maskrcnn import _hip, vis  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402


def _img(H, W, value=0.0):
    return np.full((3, H, W), value, np.float32)


def _prims(*rows):
    return np.array([tuple(r) for r in rows], ops.VIS_PRIM)


def _pixels(on):
    return sorted((int(x), int(y)) for y, x in zip(*np.nonzero(on)))


def _drawn(H, W, *rows):
    """The (x, y) pixels a white primitive list sets on a black image."""
    return _pixels(ref.render(_img(H, W), prims=_prims(*rows))[:, :, 0] == 255)


WHITE = 0xFFFFFF


# ---- blend -------------------------------------------------------------------------------------------------------------------------------
def test_blend_rule_by_hand():
    img = np.array([[[10.4, 10.5]], [[200.0, 99.6]], [[0.0, 254.5]]], np.float32)          # (3,1,2)
    rounded = np.array([[[10, 200, 0], [11, 100, 255]]], np.uint8)
    masks = np.ones((1, 1, 2), np.uint8)
    colors = np.array([[255, 0, 100]], np.uint8)
    for alpha, a in ((0.0, 0), (1.0, 256), (0.5, 128), (0.3, 77)):
        assert vis.alpha_to_a256(alpha) == a
    out = ref.render(img, masks, None, colors, None, 0, 1, ref.DRAW_MASKS)
    np.testing.assert_array_equal(out, rounded)                                          # alpha 0: the rounded image
    out = ref.render(img, masks, None, colors, None, 256, 1, ref.DRAW_MASKS)
    np.testing.assert_array_equal(out, np.broadcast_to(colors[0], (1, 2, 3)))             # alpha 1: the colour
    out = ref.render(img, masks, None, colors, None, 77, 1, ref.DRAW_MASKS)
    # a = 77: (10 * 179 + 255 * 77 + 128) >> 8 = 21553 >> 8 = 84;  (200 * 179 + 0 + 128) >> 8 = 35928 >> 8 = 140;
    #         (0 + 100 * 77 + 128) >> 8 = 7828 >> 8 = 30
    #         (11 * 179 + 255 * 77 + 128) >> 8 = 21732 >> 8 = 84;  (100 * 179 + 128) >> 8 = 18028 >> 8 = 70;
    #         (255 * 179 + 100 * 77 + 128) >> 8 = 53473 >> 8 = 208
    np.testing.assert_array_equal(out, np.array([[[84, 140, 30], [84, 70, 208]]], np.uint8))


def test_image_rounding():
    img = np.array([-3.0, -0.5, -0.4, 0.49, 0.5, 1.5, 254.49, 254.5, 255.0, 300.0, np.inf, -np.inf, np.nan], np.float32)
    want = [0, 0, 0, 0, 1, 2, 254, 255, 255, 255, 255, 0, 0]
    out = ref.render(np.broadcast_to(img, (3, 1, len(want))))
    np.testing.assert_array_equal(out[0, :, 0], want)


# ---- contour -----------------------------------------------------------------------------------------------------------------------------
def test_contour_of_a_block_and_at_the_image_edge():
    m = np.zeros((5, 5), np.uint8)
    m[1:4, 1:4] = 7                                                                      # any nonzero byte is set
    c = ref.contour(m)
    want = np.zeros((5, 5), bool)
    want[1:4, 1:4] = True
    want[2, 2] = False
    np.testing.assert_array_equal(c, want)
    assert c.sum() == 8
    full = np.ones((4, 6), np.uint8)                                                     # touches every edge: the edge is the contour
    c = ref.contour(full)
    want = np.ones((4, 6), bool)
    want[1:-1, 1:-1] = False
    np.testing.assert_array_equal(c, want)
    out = ref.render(_img(5, 5), m[None], None, np.array([[9, 8, 7]], np.uint8), None, 128, 1, ref.DRAW_CONTOURS)
    assert _pixels(out[:, :, 0] == 9) == _pixels(ref.contour(m)) and out[2, 2].tolist() == [0, 0, 0]


# ---- segments and discs ---------------------------------------------------------------------------------------------------------------------
def test_segments_of_thickness_1():
    assert _drawn(9, 9, (ops.VIS_SEGMENT, 2, 4, 6, 4, 1, WHITE, 256)) == [(x, 4) for x in range(2, 7)]
    assert _drawn(9, 9, (ops.VIS_SEGMENT, 3, 1, 3, 5, 1, WHITE, 256)) == [(3, y) for y in range(1, 6)]
    assert _drawn(9, 9, (ops.VIS_SEGMENT, 1, 2, 5, 6, 1, WHITE, 256)) == [(1 + i, 2 + i) for i in range(5)]
    assert _drawn(9, 9, (ops.VIS_SEGMENT, 6, 4, 2, 4, 1, WHITE, 256)) == [(x, 4) for x in range(2, 7)]       # the other direction


def test_segments_of_thickness_3():
    # horizontal (2,4)-(6,4): |dy| <= 1 between the ends; round caps: 4 |w|^2 <= 9 -> |w|^2 <= 2 beyond them
    want = sorted([(x, y) for x in range(1, 8) for y in (3, 4, 5)])
    assert _drawn(9, 9, (ops.VIS_SEGMENT, 2, 4, 6, 4, 3, WHITE, 256)) == want
    want = sorted([(x, y) for y in range(0, 7) for x in (2, 3, 4)])
    assert _drawn(9, 9, (ops.VIS_SEGMENT, 3, 1, 3, 5, 3, WHITE, 256)) == want
    # 45 degrees (2,2)-(5,5): between the ends 4 (wx - wy)^2 n^2 <= 9 * 2 n^2 -> |wx - wy| <= 2 with 0 < wx + wy < 6; caps |w|^2 <= 2
    want = set()
    for x in range(9):
        for y in range(9):
            wx, wy = x - 2, y - 2
            s = wx + wy
            if s <= 0:
                on = wx * wx + wy * wy <= 2
            elif s >= 6:
                on = (x - 5) ** 2 + (y - 5) ** 2 <= 2
            else:
                on = abs(wx - wy) <= 2
            if on:
                want.add((x, y))
    assert (0, 2) not in want and (1, 1) in want and (2, 4) in want and (2, 5) not in want and (3, 5) in want
    assert _drawn(9, 9, (ops.VIS_SEGMENT, 2, 2, 5, 5, 3, WHITE, 256)) == sorted(want)


def test_zero_length_segment_is_a_disc_of_the_same_width():
    # 4 |w|^2 <= t^2 with t = 2 r is |w|^2 <= r^2
    for r in (0, 1, 2, 3):
        if r:
            assert _drawn(11, 11, (ops.VIS_SEGMENT, 5, 5, 5, 5, 2 * r, WHITE, 256)) == _drawn(11, 11, (ops.VIS_DISC, 5, 5, 0, 0, r, WHITE, 256))
    assert _drawn(11, 11, (ops.VIS_DISC, 5, 5, 0, 0, 0, WHITE, 256)) == [(5, 5)]
    assert _drawn(11, 11, (ops.VIS_DISC, 5, 5, 0, 0, 1, WHITE, 256)) == [(4, 5), (5, 4), (5, 5), (5, 6), (6, 5)]
    assert len(_drawn(11, 11, (ops.VIS_DISC, 5, 5, 0, 0, 2, WHITE, 256))) == 13


def test_clipping_at_all_four_borders():
    H, W = 6, 8
    assert _drawn(H, W, (ops.VIS_DISC, 0, 0, 0, 0, 1, WHITE, 256)) == [(0, 0), (0, 1), (1, 0)]
    assert _drawn(H, W, (ops.VIS_DISC, W - 1, H - 1, 0, 0, 1, WHITE, 256)) == [(W - 2, H - 1), (W - 1, H - 2), (W - 1, H - 1)]
    assert _drawn(H, W, (ops.VIS_SEGMENT, -5, 2, 3, 2, 1, WHITE, 256)) == [(x, 2) for x in range(0, 4)]           # left
    assert _drawn(H, W, (ops.VIS_SEGMENT, 5, 2, 30, 2, 1, WHITE, 256)) == [(x, 2) for x in range(5, W)]            # right
    assert _drawn(H, W, (ops.VIS_SEGMENT, 2, -9, 2, 1, 1, WHITE, 256)) == [(2, 0), (2, 1)]                         # top
    assert _drawn(H, W, (ops.VIS_SEGMENT, 2, 4, 2, 40, 1, WHITE, 256)) == [(2, 4), (2, 5)]                         # bottom
    assert _drawn(H, W, (ops.VIS_FILL, -3, -3, 1, 0, 0, WHITE, 256)) == [(0, 0), (1, 0)]
    assert _drawn(H, W, (ops.VIS_RECT, -2, -2, 3, 2, 1, WHITE, 256)) == sorted([(3, 0), (3, 1), (3, 2), (0, 2), (1, 2), (2, 2)])
    assert _drawn(H, W, (ops.VIS_DISC, -50, -50, 0, 0, 3, WHITE, 256)) == []                                      # wholly outside
    assert _drawn(H, W, (ops.VIS_GLYPH, W - 2, H - 3, vis.UNKNOWN_GLYPH, 0, 1, WHITE, 256)) == [(x, y) for x in (W - 2, W - 1)
                                                                                              for y in range(H - 3, H)]


def test_rectangle_outline_and_glyph():
    got = _drawn(8, 8, (ops.VIS_RECT, 1, 1, 6, 5, 2, WHITE, 256))
    want = [(x, y) for x in range(1, 7) for y in range(1, 6) if not (3 <= x <= 4 and y == 3)]
    assert got == sorted(want)
    g = vis.glyph_index('t')
    out = ref.render(_img(20, 20), prims=_prims((ops.VIS_GLYPH, 3, 2, g, 0, 2, WHITE, 256)), font=vis.FONT)[:, :, 0] == 255
    np.testing.assert_array_equal(out[2:16, 3:13], np.kron(vis.glyph_bitmap(g), np.ones((2, 2), bool)))
    assert out.sum() == vis.glyph_bitmap(g).sum() * 4


def test_painters_order_in_the_reference():
    masks = np.ones((2, 3, 3), np.uint8)
    colors = np.array([[200, 0, 0], [0, 200, 0]], np.uint8)
    a = ref.render(_img(3, 3), masks, None, colors, [0, 1], 128, 1, ref.DRAW_MASKS)
    b = ref.render(_img(3, 3), masks, None, colors, [1, 0], 128, 1, ref.DRAW_MASKS)
    assert a[1, 1].tolist() == [50, 100, 0] and b[1, 1].tolist() == [100, 50, 0]         # (200 * 128 + 128) >> 8 = 100, then halved


# ---- host helpers --------------------------------------------------------------------------------------------------------------------------
def test_palette():
    p = vis.palette(80)
    assert p.dtype == np.uint8 and p.shape == (80, 3)
    assert len({tuple(c) for c in p.tolist()}) == 80
    np.testing.assert_array_equal(p, vis.palette(80))
    np.testing.assert_array_equal(p[:7], vis.palette(7))
    assert vis.palette(0).shape == (0, 3)
    assert len({tuple(c) for c in vis.palette(300).tolist()}) == 300


def test_font():
    need = 'abcdefghijklmnopqrstuvwxyz0123456789.%-_ '
    assert vis.FONT.dtype == np.uint64 and len(vis.FONT) == len(vis.FONT_CHARS) + 1 <= ops.VIS_GLYPHS_MAX
    for ch in need:
        g = vis.glyph_index(ch)
        assert g != vis.UNKNOWN_GLYPH, ch
        assert int(vis.FONT[g]) < 1 << 35                                                # fits 5 x 7
        assert vis.glyph_bitmap(g).shape == (7, 5)
        assert (int(vis.FONT[g]) == 0) == (ch == ' ')
    assert all(len(rows) == 7 and all(len(r) == 5 and set(r) <= {'#', '.'} for r in rows) for rows in vis._FONT_ROWS.values())
    assert len({int(b) for b in vis.FONT}) == len(vis.FONT)                              # no two characters look alike
    assert vis.glyph_index('A') == vis.glyph_index('a')
    assert vis.glyph_index('#') == vis.UNKNOWN_GLYPH and vis.glyph_bitmap(vis.UNKNOWN_GLYPH).all()


def test_label_text_and_luminance():
    assert vis.label_text(2, 0.98765, ['person', 'bicycle', 'car']) == 'car 0.99'
    assert vis.label_text(1, 0.5, None) == '1 0.50'
    assert vis.label_text(7, 1.0, ['a']) == '7 1.00'
    assert vis.luminance((255, 255, 255)) == 255 and vis.luminance((0, 0, 0)) == 0 and vis.luminance((0, 255, 0)) == 149
    assert vis.text_size('ab', 2) == ((2 * 5 + 1 + 2) * 2, 9 * 2)


def test_draw_order_is_ascending_and_stable():
    np.testing.assert_array_equal(vis.draw_order([0.9, 0.2, 0.9, 0.2, 0.5]), [1, 3, 4, 0, 2])
    assert vis.draw_order([]).shape == (0,) and vis.draw_order([0.3]).dtype == np.int32


def test_instance_primitives():
    bboxes = np.array([[10.4, 20.6, 60, 90], [-5, -7, 30, 30], [90, 95, 99, 99]], np.float32)
    labels, scores = np.array([2, 0, 1]), np.array([0.9, 0.8, 0.95], np.float32)
    names = ['person', 'bicycle', 'car']
    order, colors, prims = vis.instance_primitives(100, 100, bboxes, labels, scores, names, 'class', True, 1)
    np.testing.assert_array_equal(order, [1, 0, 2])
    assert colors.dtype == np.uint8 and colors.shape == (3, 3)
    np.testing.assert_array_equal(colors, vis.palette(3)[labels])
    assert prims.dtype == ops.VIS_PRIM and prims.dtype.itemsize == 32 and prims.ndim == 1
    texts = ['person 0.80', 'car 0.90', 'bicycle 0.95']
    assert len(prims) == sum(1 + len(t) for t in texts)
    ops.check_vis_prims(prims)
    i = 0
    for d, t in zip(order, texts):
        bg = prims[i]
        tw, th = vis.text_size(t, 1)
        assert bg['kind'] == ops.VIS_FILL and bg['rgb'] == vis.pack_rgb(colors[d]) and bg['a'] == 256
        assert bg['x1'] - bg['x0'] + 1 == tw and bg['y1'] - bg['y0'] + 1 == th
        assert 0 <= bg['x0'] and bg['x1'] < 100 and 0 <= bg['y0'] and bg['y1'] < 100                 # moved into the image
        ink = 0xFFFFFF if vis.luminance(colors[d]) < 128 else 0
        for k, ch in enumerate(t):
            g = prims[i + 1 + k]
            assert (g['kind'], g['x1'], g['p'], g['rgb']) == (ops.VIS_GLYPH, vis.glyph_index(ch), 1, ink)
            assert (g['x0'], g['y0']) == (bg['x0'] + 1 + 6 * k, bg['y0'] + 1)
        i += 1 + len(t)
    assert (prims[len(texts[0]) + 1]['x0'], prims[len(texts[0]) + 1]['y0']) == (21, 10)                # floor(20.6 + .5), floor(10.4 + .5)
    assert (prims[0]['x0'], prims[0]['y0']) == (0, 0)
    _, by_instance, none = vis.instance_primitives(100, 100, bboxes, labels, scores, names, 'instance', False, 1)
    np.testing.assert_array_equal(by_instance, vis.palette(3))
    assert none.shape == (0,) and none.dtype == ops.VIS_PRIM
    o, c, p = vis.instance_primitives(50, 50, np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert o.shape == (0,) and c.shape == (0, 3) and p.shape == (0,)
    with pytest.raises(ValueError):
        vis.instance_primitives(50, 50, bboxes, labels, scores, color_by='size')
    with pytest.raises(ValueError):
        vis.instance_primitives(50, 50, bboxes, labels[:2], scores)


def test_keypoint_primitives():
    assert len(vis.COCO_PERSON_SKELETON) == 19 and all(0 <= a < 17 and 0 <= b < 17 and a != b for a, b in vis.COCO_PERSON_SKELETON)
    assert len(set(map(frozenset, vis.COCO_PERSON_SKELETON))) == 19
    rs = np.random.RandomState(0)
    kp = np.zeros((2, 17, 4), np.float32)
    kp[:, :, :2] = rs.uniform(0, 60, (2, 17, 2))
    kp[:, :, 2] = 5.0
    kp[:, :, 3] = 0.5
    kp[0, 5, 2] = 1.0                                                                    # left shoulder of instance 0 below the threshold
    boxes, scores = np.array([[0, 0, 50, 50], [10, 10, 60, 60]], np.float32), np.array([0.9, 0.4], np.float32)
    prims = vis.keypoint_primitives(kp, boxes, scores, kp_thresh=2.0, on='logit', radius=3, thickness=2, alpha=0.5)
    assert prims.dtype == ops.VIS_PRIM
    limbs_with_5 = sum(1 for a, b in vis.COCO_PERSON_SKELETON if 5 in (a, b))
    assert len(prims) == 2 + (19 + 17) + (19 - limbs_with_5 + 16)
    assert [int(k) for k in prims['kind'][:2]] == [ops.VIS_RECT, ops.VIS_SEGMENT]
    first = prims[0]                                                                     # instance 1 (the lower score) is drawn first
    assert (first['x0'], first['y0'], first['x1'], first['y1']) == (10, 10, 60, 60)
    seg = prims[1]
    a, b = vis.COCO_PERSON_SKELETON[0]
    want = [int(np.floor(kp[1, a, 1] + np.float32(0.5))), int(np.floor(kp[1, a, 0] + np.float32(0.5))),
            int(np.floor(kp[1, b, 1] + np.float32(0.5))), int(np.floor(kp[1, b, 0] + np.float32(0.5)))]
    assert [seg['x0'], seg['y0'], seg['x1'], seg['y1']] == want and seg['p'] == 2 and seg['a'] == 128
    assert seg['rgb'] == vis.pack_rgb(vis.palette(19)[0])
    discs = prims[prims['kind'] == ops.VIS_DISC]
    assert len(discs) == 33 and set(discs['p'].tolist()) == {3}
    on_prob = vis.keypoint_primitives(kp, boxes, scores, kp_thresh=0.6, on='prob', draw_boxes=False)
    assert len(on_prob) == 0
    dots = vis.keypoint_primitives(kp[:, :5], boxes, scores, kp_thresh=2.0)              # K != 17: dots only
    assert set(dots['kind'].tolist()) == {ops.VIS_RECT, ops.VIS_DISC} and (dots['kind'] == ops.VIS_DISC).sum() == 10
    own = vis.keypoint_primitives(kp[:, :5], boxes, scores, skeleton=[(0, 1), (3, 4)], kp_thresh=2.0)
    assert (own['kind'] == ops.VIS_SEGMENT).sum() == 4
    with pytest.raises(ValueError):
        vis.keypoint_primitives(kp[:, :5], boxes, scores, skeleton=[(0, 5)])
    with pytest.raises(ValueError):
        vis.keypoint_primitives(kp, boxes, scores, on='heat')


def test_primitive_caps_are_checked_on_the_host():
    ok = _prims((ops.VIS_DISC, 5, 5, 0, 0, 0, 0, 256), (ops.VIS_SEGMENT, -4096, 20479, 0, 0, 4096, WHITE, 0))
    assert ops.check_vis_prims(ok).shape == (2,)
    assert ops.check_vis_prims(np.zeros((0, 8), np.int32)).shape == (0,)
    for bad in ((ops.VIS_DISC, 20480, 0, 0, 0, 1, 0, 256), (ops.VIS_SEGMENT, 0, 0, 0, -4097, 1, 0, 256), (5, 0, 0, 0, 0, 1, 0, 256),
                (ops.VIS_RECT, 0, 0, 4, 4, 0, 0, 256), (ops.VIS_GLYPH, 0, 0, 0, 0, 65, 0, 256), (ops.VIS_FILL, 0, 0, 1, 1, 0, 0, 257),
                (ops.VIS_DISC, 0, 0, 0, 0, 4097, 0, 256), (ops.VIS_FILL, 0, 0, 1, 1, 0, 1 << 24, 256)):
        with pytest.raises(ValueError, match='row 1'):
            ops.check_vis_prims(_prims(ok[0], bad))
        with pytest.raises(ValueError):
            ref.render(_img(4, 4), prims=_prims(bad))
    with pytest.raises(ValueError):
        ops.check_vis_prims(np.zeros((3, 7), np.int32))


# ---- demo.py -------------------------------------------------------------------------------------------------------------------------------
def test_demo_parser_defaults():
    import demo
    a = demo.build_parser().parse_args([])
    assert a.inputs == [] and a.synthetic == 0 and a.weight == '' and a.label_file == 'data/label_coco.txt'
    assert a.backbone == 'fpn' and a.head_arch == 'fpn' and a.gpu == 0 and a.out == 'result_demo'
    assert a.score_thresh is None and a.alpha == 0.5 and a.color_by == 'class' and a.kp_thresh is None
    assert not (a.no_masks or a.no_boxes or a.no_labels or a.no_contours)
    assert a.tta_sizes is None and a.tta_hflip == 0 and a.tta_max_size is None and a.json == 0 and a.image_size == [480, 640]
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    m = MaskRCNN(n_fg_class=80, device='cpu', _test_shrink=dict(stages=(1, 1, 1, 1), width_div=4))
    m.use_preset('visualize')
    assert m.score_thresh == demo.VISUALIZE_SCORE_THRESH
    a = demo.build_parser().parse_args(['x.png', 'dir', '--no-masks', '--json', '1', '--image-size', '96', '128', '--color-by', 'instance'])
    assert a.inputs == ['x.png', 'dir'] and a.no_masks and a.json == 1 and a.image_size == [96, 128] and a.color_by == 'instance'
    for name in ('build_parser', 'check_args', 'run', 'main'):
        assert callable(getattr(demo, name))


def test_demo_refusals_come_before_the_model(monkeypatch, tmp_path):
    import demo
    from PIL import Image
    monkeypatch.setattr(demo, 'build_model', lambda args: pytest.fail('the model was built'))
    parse = demo.build_parser().parse_args
    (tmp_path / 'imgs').mkdir()
    good = tmp_path / 'imgs' / 'good.png'
    Image.fromarray(np.zeros((4, 5, 3), np.uint8)).save(str(good))
    empty_dir = tmp_path / 'empty'
    empty_dir.mkdir()
    empty_file = tmp_path / 'empty.png'
    empty_file.write_bytes(b'')
    text = tmp_path / 'notes.jpg'
    text.write_text('not an image')
    for argv in ([], [str(tmp_path / 'missing.png')], [str(empty_dir)], [str(empty_file)], [str(text)], [str(good), '--synthetic', '2'],
                 ['--synthetic', '-1'], ['--synthetic', '1', '--alpha', '1.5'], ['--synthetic', '1', '--image-size', '0', '10'],
                 ['--synthetic', '1', '--kp-thresh', '2'], ['--synthetic', '1', '--head-arch', 'fpn_keypoint', '--no-masks'],
                 ['--synthetic', '1', '--head-arch', 'fpn_keypoint', '--no-contours'],
                 ['--synthetic', '1', '--head-arch', 'fpn_keypoint', '--no-labels'],
                 ['--synthetic', '1', '--head-arch', 'fpn_keypoint', '--color-by', 'instance'],
                 ['--synthetic', '1', '--tta-max-size', '500'], ['--synthetic', '1', '--tta-sizes', '0'],
                 ['--synthetic', '1', '--score-thresh', '2']):
        with pytest.raises(ValueError):
            demo.run(parse(argv + ['--out', str(tmp_path / 'out')]))
    assert not (tmp_path / 'out').exists()
    assert demo.check_args(parse([str(good), str(tmp_path / 'imgs')])) == [str(good), str(good)]
    assert demo.check_args(parse(['--synthetic', '3', '--head-arch', 'fpn_keypoint', '--no-boxes', '--kp-thresh', '1'])) == []
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='single process'):
        demo.run(parse(['--synthetic', '1']))


# ---- the entry point and the package ---------------------------------------------------------------------------------------------------------
def test_argument_errors_do_not_need_a_device():
    lib = _hip.lib()
    buf = (ctypes.c_char * 4096)()                    # host memory standing in for device buffers: no call below reaches a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def call(img=p, H=4, W=4, masks=p, bbox=p, colors=p, order=None, D=1, a=128, t=1, flags=7, prims=p, n_prims=1, font=p, n_glyphs=1,
             out=p):
        return lib.mrcnn_vis_render_u8(img, H, W, masks, bbox, colors, order, D, a, t, flags, prims, n_prims, font, n_glyphs, out, None)
    cases = [(dict(img=None), b'img'), (dict(out=None), b'out'), (dict(masks=None), b'masks'), (dict(bbox=None), b'bbox'),
             (dict(colors=None), b'colors'), (dict(prims=None), b'prims'), (dict(font=None), b'font'), (dict(H=-1), b'H'),
             (dict(W=-2), b'W'), (dict(H=16385), b'H'), (dict(W=16385), b'W'), (dict(D=-1), b'D'), (dict(n_prims=-1), b'n_prims'),
             (dict(n_glyphs=257), b'n_glyphs'), (dict(a=257), b'mask_a256'), (dict(a=-1), b'mask_a256'), (dict(t=0), b'box_thickness'),
             (dict(t=4097), b'box_thickness'), (dict(flags=8), b'flags'), (dict(prims=p + 4), b'prims'), (dict(order=p + 1), b'order'),
             (dict(img=p + 2), b'img')]
    for kw, word in cases:
        rc = call(**kw)
        assert rc == -1, kw
        assert word in lib.mrcnn_last_error(), (kw, lib.mrcnn_last_error())
        with pytest.raises(_hip.MrcnnHipError):
            _hip.check(rc)
    assert call(H=0) == 0 and call(W=0, img=None, out=None) == 0                         # no pixels: a no-op, nothing is launched
    import torch
    with pytest.raises(_hip.MrcnnHipError):                                              # no CPU fallback
        ops.vis_render(torch.zeros(3, 4, 4))
    sig = _hip.SIGNATURES['mrcnn_vis_render_u8']
    assert sig[0] is ctypes.c_int and len(sig[1]) == 17 and sig[1][-1] is ctypes.c_void_p


def test_header_and_binding_agree_on_the_caps():
    src = open(_hip.HEADER_PATH).read()
    defs = {k: int(v.strip('()')) for k, v in re.findall(r'#define (MRCNN_VIS_[A-Z_0-9]+) (\(?-?\d+\)?)', src)}
    assert defs['MRCNN_VIS_MAX_SIDE'] == ops.VIS_MAX_SIDE == ref.MAX_SIDE == 16384
    assert (defs['MRCNN_VIS_COORD_MIN'], defs['MRCNN_VIS_COORD_MAX']) == (ops.VIS_COORD_MIN, ops.VIS_COORD_MAX) == (ref.COORD_MIN, ref.COORD_MAX)
    assert defs['MRCNN_VIS_PARAM_MAX'] == ops.VIS_PARAM_MAX == ref.PARAM_MAX
    assert defs['MRCNN_VIS_GLYPH_SCALE_MAX'] == ops.VIS_GLYPH_SCALE_MAX == ref.GLYPH_SCALE_MAX
    assert defs['MRCNN_VIS_GLYPHS_MAX'] == ops.VIS_GLYPHS_MAX
    assert [defs['MRCNN_VIS_' + k] for k in ('RECT', 'SEGMENT', 'DISC', 'GLYPH', 'FILL')] == [0, 1, 2, 3, 4] == \
        [ops.VIS_RECT, ops.VIS_SEGMENT, ops.VIS_DISC, ops.VIS_GLYPH, ops.VIS_FILL]
    assert (defs['MRCNN_VIS_DRAW_MASKS'], defs['MRCNN_VIS_DRAW_CONTOURS'], defs['MRCNN_VIS_DRAW_BOXES']) == (1, 2, 4)
    assert (defs['MRCNN_VIS_GLYPH_W'], defs['MRCNN_VIS_GLYPH_H']) == (vis.GLYPH_W, vis.GLYPH_H)
    # the segment rule stays inside int64: |w|, |d| components <= R = COORD_MAX - COORD_MIN, |cross| <= 2 R^2, 4 cross^2 <= 16 R^4
    R = ops.VIS_COORD_MAX - ops.VIS_COORD_MIN
    assert 16 * R ** 4 < 2 ** 63 and ops.VIS_PARAM_MAX ** 2 * 2 * R ** 2 < 2 ** 63 and ops.VIS_MAX_SIDE - 1 <= ops.VIS_COORD_MAX


def test_product_does_not_import_tests_or_oracle():
    pkg = os.path.join(ROOT, 'chainer-maskrcnn_amd')
    paths = [os.path.join(dp, fn) for dp, _, fns in os.walk(pkg) for fn in fns if fn.endswith('.py')] + [os.path.join(ROOT, 'demo.py')]
    assert any(p.endswith(os.path.join('chainer_maskrcnn', 'vis.py')) for p in paths)
    for p in paths:
        txt = open(p).read()
        assert not re.search(r'^\s*(from|import)\s+(oracle|tests|vis_reference)\b', txt, flags=re.M), p
