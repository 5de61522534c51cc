"""Pictures of detections: masks, contours, boxes, labels and keypoint skeletons drawn on the device by ``mrcnn_vis_render_u8``
(csrc/vis.hip).  This module is the host half: the palette, the bitmap font, the drawing order and the primitive
array; none of it needs a device except the final call in ``draw_instances`` / ``draw_keypoints``.

The raster rule is this project's own: integer-only, no anti-aliasing, every pixel a pure function of the inputs, so that a NumPy
restatement reproduces a picture bit for bit.  It is not the rule of the model project's vis.py / viewer.py (cv2 drawing with
anti-aliasing), whose pictures it therefore does not reproduce; the palette, the font and the default skeleton are not taken from there
either (the skeleton is the ``skeleton`` field of COCO's public person_keypoints annotation files).
"""
import numpy as np

from chainer_maskrcnn._hip import ops
from chainer_maskrcnn._hip.ops import VIS_PRIM, VIS_RECT, VIS_SEGMENT, VIS_DISC, VIS_GLYPH, VIS_FILL

GLYPH_W, GLYPH_H = 5, 7

# 5 x 7 bitmap font: seven rows of five cells per character, '#' = set.  Letters are drawn as small capitals.
_FONT_ROWS = {
    ' ': ('.....', '.....', '.....', '.....', '.....', '.....', '.....'),
    'a': ('.###.', '#...#', '#...#', '#####', '#...#', '#...#', '#...#'),
    'b': ('####.', '#...#', '#...#', '####.', '#...#', '#...#', '####.'),
    'c': ('.###.', '#...#', '#....', '#....', '#....', '#...#', '.###.'),
    'd': ('####.', '#...#', '#...#', '#...#', '#...#', '#...#', '####.'),
    'e': ('#####', '#....', '#....', '####.', '#....', '#....', '#####'),
    'f': ('#####', '#....', '#....', '####.', '#....', '#....', '#....'),
    'g': ('.###.', '#...#', '#....', '#.###', '#...#', '#...#', '.####'),
    'h': ('#...#', '#...#', '#...#', '#####', '#...#', '#...#', '#...#'),
    'i': ('.###.', '..#..', '..#..', '..#..', '..#..', '..#..', '.###.'),
    'j': ('..###', '...#.', '...#.', '...#.', '...#.', '#..#.', '.##..'),
    'k': ('#...#', '#..#.', '#.#..', '##...', '#.#..', '#..#.', '#...#'),
    'l': ('#....', '#....', '#....', '#....', '#....', '#....', '#####'),
    'm': ('#...#', '##.##', '#.#.#', '#.#.#', '#...#', '#...#', '#...#'),
    'n': ('#...#', '##..#', '#.#.#', '#..##', '#...#', '#...#', '#...#'),
    'o': ('.###.', '#...#', '#...#', '#...#', '#...#', '#...#', '.###.'),
    'p': ('####.', '#...#', '#...#', '####.', '#....', '#....', '#....'),
    'q': ('.###.', '#...#', '#...#', '#...#', '#.#.#', '#..#.', '.##.#'),
    'r': ('####.', '#...#', '#...#', '####.', '#.#..', '#..#.', '#...#'),
    's': ('.####', '#....', '#....', '.###.', '....#', '....#', '####.'),
    't': ('#####', '..#..', '..#..', '..#..', '..#..', '..#..', '..#..'),
    'u': ('#...#', '#...#', '#...#', '#...#', '#...#', '#...#', '.###.'),
    'v': ('#...#', '#...#', '#...#', '#...#', '#...#', '.#.#.', '..#..'),
    'w': ('#...#', '#...#', '#...#', '#.#.#', '#.#.#', '##.##', '#...#'),
    'x': ('#...#', '#...#', '.#.#.', '..#..', '.#.#.', '#...#', '#...#'),
    'y': ('#...#', '#...#', '.#.#.', '..#..', '..#..', '..#..', '..#..'),
    'z': ('#####', '....#', '...#.', '..#..', '.#...', '#....', '#####'),
    '0': ('.###.', '#...#', '#..##', '#.#.#', '##..#', '#...#', '.###.'),
    '1': ('..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.'),
    '2': ('.###.', '#...#', '....#', '...#.', '..#..', '.#...', '#####'),
    '3': ('####.', '....#', '....#', '.###.', '....#', '....#', '####.'),
    '4': ('...#.', '..##.', '.#.#.', '#..#.', '#####', '...#.', '...#.'),
    '5': ('#####', '#....', '####.', '....#', '....#', '#...#', '.###.'),
    '6': ('..##.', '.#...', '#....', '####.', '#...#', '#...#', '.###.'),
    '7': ('#####', '....#', '...#.', '..#..', '.#...', '.#...', '.#...'),
    '8': ('.###.', '#...#', '#...#', '.###.', '#...#', '#...#', '.###.'),
    '9': ('.###.', '#...#', '#...#', '.####', '....#', '...#.', '.##..'),
    '.': ('.....', '.....', '.....', '.....', '.....', '.##..', '.##..'),
    '%': ('##...', '##..#', '...#.', '..#..', '.#...', '#..##', '...##'),
    '-': ('.....', '.....', '.....', '#####', '.....', '.....', '.....'),
    '_': ('.....', '.....', '.....', '.....', '.....', '.....', '#####'),
}
FONT_CHARS = ''.join(sorted(_FONT_ROWS))
UNKNOWN_GLYPH = len(FONT_CHARS)                  # the last glyph: a filled cell


def _glyph_bits(rows):
    return sum(1 << (GLYPH_W * r + c) for r in range(GLYPH_H) for c in range(GLYPH_W) if rows[r][c] == '#')


# bit 5 * row + col of FONT[g] = cell (row, col) of glyph g, as mrcnn_vis_render_u8 takes the font
FONT = np.array([_glyph_bits(_FONT_ROWS[ch]) for ch in FONT_CHARS] + [(1 << (GLYPH_W * GLYPH_H)) - 1], np.uint64)


def glyph_index(ch):
    """The glyph of a character (letters fold to one case); UNKNOWN_GLYPH, the filled cell, for a character the font lacks."""
    i = FONT_CHARS.find(ch.lower()) if len(ch) == 1 else -1
    return i if i >= 0 else UNKNOWN_GLYPH


def glyph_bitmap(g):
    """(7,5) bool cells of glyph g."""
    bits = int(FONT[g])
    return np.array([[(bits >> (GLYPH_W * r + c)) & 1 for c in range(GLYPH_W)] for r in range(GLYPH_H)], bool)


def palette_color(i):
    """Colour i of the palette as (r, g, b) ints: the hue walks the colour circle in steps of 137 degrees (coprime to 360, so 360
    different hues), the value alternates between two levels every 12 colours; integer HSV -> RGB with the minimum channel at value / 5."""
    i = int(i)
    h = (i * 137) % 360
    v = (255, 205)[(i // 12) % 2]
    m = v // 5
    x = m + (v - m) * (60 - abs(h % 120 - 60)) // 60
    return ((v, x, m), (x, v, m), (m, v, x), (m, x, v), (x, m, v), (v, m, x))[h // 60]


def palette(n):
    """n distinct uint8 RGB colours, (n,3), from the fixed formula of ``palette_color``; palette(n)[:k] == palette(k)."""
    return np.array([palette_color(i) for i in range(n)], np.uint8).reshape(n, 3)


def luminance(rgb):
    """Integer luminance 0..255 of an (r, g, b) colour: (299 r + 587 g + 114 b) // 1000."""
    r, g, b = (int(c) for c in rgb)
    return (299 * r + 587 * g + 114 * b) // 1000


def pack_rgb(rgb):
    r, g, b = (int(c) for c in rgb)
    return r | (g << 8) | (b << 16)


def alpha_to_a256(alpha):
    """round(alpha * 256) in [0, 256], halves upwards."""
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError('alpha must lie in [0, 1], got %r' % (alpha,))
    return int(np.floor(a * 256 + 0.5))


def round_coords(v):
    """floor(v + 0.5) in float32, clamped to the renderer's coordinate range (NaN: its lower end), as int32 - the kernel's rule for boxes."""
    q = np.floor(np.asarray(v, np.float32) + np.float32(0.5))
    with np.errstate(invalid='ignore'):
        r = np.where(q >= ops.VIS_COORD_MAX, ops.VIS_COORD_MAX, np.where(q > ops.VIS_COORD_MIN, q, ops.VIS_COORD_MIN))
    return r.astype(np.int32)


def draw_order(scores):
    """Indices in ascending score order, ties in input order: the highest-scoring instance is drawn last and ends on top."""
    return np.argsort(np.asarray(scores, np.float32).reshape(-1), kind='stable').astype(np.int32)


def label_text(label, score, label_names=None):
    """"<name> <score to 2 decimals>"; the class index stands in for a missing name."""
    label = int(label)
    name = label_names[label] if label_names is not None and 0 <= label < len(label_names) else str(label)
    return '%s %.2f' % (name, float(score))


def _prim(kind, x0, y0, x1=0, y1=0, p=0, rgb=0, a=256):
    return (int(kind), int(x0), int(y0), int(x1), int(y1), int(p), int(rgb), int(a))


def text_primitives(text, x0, y0, scale, rgb):
    """One glyph cell per character from (x0, y0), advancing (GLYPH_W + 1) * scale per character."""
    return [_prim(VIS_GLYPH, x0 + i * (GLYPH_W + 1) * scale, y0, glyph_index(ch), 0, scale, rgb) for i, ch in enumerate(text)]


def text_size(text, scale):
    """(width, height) of the label background of a text: the cells, the gaps between them and a margin of `scale` on every side."""
    n = len(text)
    return (n * GLYPH_W + max(n - 1, 0) + 2) * scale, (GLYPH_H + 2) * scale


def _host(a, dtype):
    if a is None:
        return None
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype)


def instance_primitives(H, W, bboxes, labels, scores, label_names=None, color_by='class', draw_labels=True, font_scale=1):
    """The host half of ``draw_instances`` (no device): returns (order, colors, prims).  order (D,) int32 = ``draw_order(scores)``;
    colors (D,3) uint8 per instance in INPUT order - palette colour of the class (color_by 'class') or of the input index ('instance');
    prims: VIS_PRIM array, per instance in drawing order a label background (a filled rectangle in the instance colour with its top-left at
    the box's rounded top-left, moved into the image) and the glyph cells of ``label_text`` in black or white, white where the
    background's ``luminance`` is below 128.  Empty with draw_labels off."""
    if color_by not in ('class', 'instance'):
        raise ValueError("color_by must be 'class' or 'instance', got %r" % (color_by,))
    font_scale = int(font_scale)
    if not 1 <= font_scale <= ops.VIS_GLYPH_SCALE_MAX:
        raise ValueError('font_scale must lie in 1..%d, got %d' % (ops.VIS_GLYPH_SCALE_MAX, font_scale))
    bboxes, labels, scores = _host(bboxes, np.float32).reshape(-1, 4), _host(labels, np.int64).reshape(-1), _host(scores, np.float32).reshape(-1)
    D = labels.shape[0]
    if bboxes.shape[0] != D or scores.shape[0] != D:
        raise ValueError('draw_instances: %d boxes, %d labels, %d scores' % (bboxes.shape[0], D, scores.shape[0]))
    order = draw_order(scores)
    colors = np.array([palette_color(labels[d] if color_by == 'class' else d) for d in range(D)], np.uint8).reshape(D, 3)
    rows = []
    if draw_labels:
        corners = round_coords(bboxes)
        for d in order:
            text = label_text(labels[d], scores[d], label_names)
            tw, th = text_size(text, font_scale)
            x0 = min(max(int(corners[d, 1]), 0), max(W - tw, 0))
            y0 = min(max(int(corners[d, 0]), 0), max(H - th, 0))
            rows.append(_prim(VIS_FILL, x0, y0, x0 + tw - 1, y0 + th - 1, 0, pack_rgb(colors[d])))
            ink = 0xFFFFFF if luminance(colors[d]) < 128 else 0
            rows += text_primitives(text, x0 + font_scale, y0 + font_scale, font_scale, ink)
    return order, colors, np.array(rows, VIS_PRIM).reshape(-1)


def draw_instances(img, masks, bboxes, labels, scores, label_names=None, alpha=0.5, color_by='class', draw_masks=True, draw_boxes=True,
                   draw_labels=True, draw_contours=True, thickness=2, font_scale=1):
    """The picture of one image's detections: img (3,H,W) float32 RGB 0..255 and masks (D,H,W) bool / uint8 on the device as ``predict``
    takes / returns them, bboxes (D,4) (y1,x1,y2,x2) (``model.last_bboxes``), labels (D,), scores (D,).  Returns an (H,W,3) uint8 RGB
    device tensor (PIL's layout); the caller makes the one device->host copy.
    Instances are drawn in ascending score order, ties in input order - part of the contract: the best detection ends on top.  Per
    instance its mask blended with ``alpha``, its contour, its box outline (``thickness``); after all instances the labels.  The raster
    rules are the renderer's own integer rules, not cv2's: no anti-aliasing, bit-exact against NumPy."""
    H, W = int(img.shape[1]), int(img.shape[2])
    order, colors, prims = instance_primitives(H, W, bboxes, labels, scores, label_names, color_by, draw_labels, font_scale)
    flags = (ops.VIS_DRAW_MASKS if draw_masks else 0) | (ops.VIS_DRAW_CONTOURS if draw_contours else 0) | \
        (ops.VIS_DRAW_BOXES if draw_boxes else 0)
    D = order.shape[0]
    if masks is not None and int(masks.shape[0]) != D:
        raise ValueError('draw_instances: %d masks for %d detections' % (int(masks.shape[0]), D))
    if masks is None:
        flags &= ~(ops.VIS_DRAW_MASKS | ops.VIS_DRAW_CONTOURS)
    bb = None
    if draw_boxes and D:
        import torch
        bb = bboxes if hasattr(bboxes, 'is_cuda') else torch.from_numpy(_host(bboxes, np.float32).reshape(-1, 4))
        bb = bb.to(img.device)
    return ops.vis_render(img, masks if flags & 3 else None, bb, colors, order, alpha_to_a256(alpha), int(thickness), flags, prims, FONT)


# COCO's person skeleton: the `skeleton` field of the person category in the public person_keypoints annotation files (1-based there)
COCO_PERSON_SKELETON = tuple((a - 1, b - 1) for a, b in (
    (16, 14), (14, 12), (17, 15), (15, 13), (12, 13), (6, 12), (7, 13), (6, 7), (6, 8), (7, 9), (8, 10), (9, 11), (2, 3), (1, 2), (1, 3),
    (2, 4), (3, 5), (4, 6), (5, 7)))


def keypoint_primitives(keypoints, bboxes, scores, skeleton=None, kp_thresh=2.0, on='logit', radius=3, thickness=2, alpha=1.0,
                        draw_boxes=True):
    """The host half of ``draw_keypoints`` (no device): the VIS_PRIM array.  Instances in ``draw_order(scores)``; per instance its box
    outline (palette colour of the input index, opaque), then its limbs, then its keypoints.  A keypoint is drawn, as a disc of
    ``radius`` in palette(K)[k], when its score (column 3 'prob' or column 2 'logit' of keypoints) is >= kp_thresh; a limb, as a segment
    of ``thickness`` in palette(len(skeleton))[l], when both of its ends are drawn.  Coordinates are floor(v + 0.5).  Limbs and discs are
    blended with ``alpha``.  The COCO person skeleton is the default for K == 17 only; any other K draws dots unless a skeleton is given."""
    if on not in ('prob', 'logit'):
        raise ValueError("on must be 'prob' or 'logit', got %r" % (on,))
    kp = _host(keypoints, np.float32)
    if kp.ndim != 3 or kp.shape[2] != 4:
        raise ValueError('draw_keypoints: keypoints (D,K,4) expected, got %s' % (kp.shape,))
    D, K = kp.shape[:2]
    bboxes, scores = _host(bboxes, np.float32).reshape(-1, 4), _host(scores, np.float32).reshape(-1)
    if bboxes.shape[0] != D or scores.shape[0] != D:
        raise ValueError('draw_keypoints: %d instances, %d boxes, %d scores' % (D, bboxes.shape[0], scores.shape[0]))
    if skeleton is None:
        skeleton = COCO_PERSON_SKELETON if K == 17 else ()
    skeleton = [(int(a), int(b)) for a, b in skeleton]
    if any(not (0 <= a < K and 0 <= b < K) for a, b in skeleton):
        raise ValueError('draw_keypoints: a limb names a keypoint outside 0..%d' % (K - 1))
    a256 = alpha_to_a256(alpha)
    yx = round_coords(kp[:, :, :2])
    with np.errstate(invalid='ignore'):
        shown = kp[:, :, 3 if on == 'prob' else 2] >= np.float32(kp_thresh)
    corners = round_coords(bboxes)
    limb_rgb = [pack_rgb(c) for c in palette(len(skeleton))]
    dot_rgb = [pack_rgb(c) for c in palette(K)]
    rows = []
    for d in draw_order(scores):
        if draw_boxes:
            top, left, bottom, right = (int(v) for v in corners[d])
            rows.append(_prim(VIS_RECT, left, top, right, bottom, max(1, int(thickness) // 2), pack_rgb(palette_color(d))))
        for l, (a, b) in enumerate(skeleton):
            if shown[d, a] and shown[d, b]:
                rows.append(_prim(VIS_SEGMENT, yx[d, a, 1], yx[d, a, 0], yx[d, b, 1], yx[d, b, 0], thickness, limb_rgb[l], a256))
        for k in range(K):
            if shown[d, k]:
                rows.append(_prim(VIS_DISC, yx[d, k, 1], yx[d, k, 0], 0, 0, radius, dot_rgb[k], a256))
    return np.array(rows, VIS_PRIM).reshape(-1)


def draw_keypoints(img, keypoints, bboxes, scores, skeleton=None, kp_thresh=2.0, on='logit', radius=3, thickness=2, alpha=1.0,
                   draw_boxes=True):
    """The picture of one image's keypoint detections: keypoints (D,K,4) (y, x, logit, prob) as ``predict_keypoints`` returns them,
    bboxes (D,4) (``model.last_bboxes``), scores (D,).  Returns an (H,W,3) uint8 RGB device tensor.  What is drawn and in which order:
    ``keypoint_primitives``.  The raster rules are the renderer's own integer rules, not cv2's."""
    prims = keypoint_primitives(keypoints, bboxes, scores, skeleton, kp_thresh, on, radius, thickness, alpha, draw_boxes)
    return ops.vis_render(img, prims=prims, font=FONT)
