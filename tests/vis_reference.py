"""NumPy restatement of the renderer's contract (include/mrcnn_hip.h mrcnn_vis_render_u8), written from the
contract in whole-array operations: one boolean (H,W) coverage array per instance layer and per primitive, composed with np.where in
painter's order.  A helper of the tests (tests/test_vis_cpu.py, tests/test_vis_gpu.py) and of tools/vis_bench.py, not a test and not
part of the product.  ``render`` takes the arguments of ``chainer_maskrcnn._hip.ops.vis_render`` as host arrays."""
import numpy as np

RECT, SEGMENT, DISC, GLYPH, FILL = range(5)
DRAW_MASKS, DRAW_CONTOURS, DRAW_BOXES = 1, 2, 4
COORD_MIN, COORD_MAX, PARAM_MAX, GLYPH_SCALE_MAX, MAX_SIDE = -4096, 20479, 4096, 64, 16384
FIELDS = ('kind', 'x0', 'y0', 'x1', 'y1', 'p', 'rgb', 'a')


def round_image(img):
    """(3,H,W) float32 -> (H,W,3) int64 of min(255, max(0, floor(v + 0.5))), NaN -> 0."""
    q = np.floor(np.asarray(img, np.float32) + np.float32(0.5))
    q = np.where(np.isnan(q), np.float32(0), q)
    return np.clip(q, 0, 255).astype(np.int64).transpose(1, 2, 0)


def blend(c, col, a):
    """(c * (256 - a) + col * a + 128) >> 8 on int64 arrays."""
    return (c * (256 - a) + np.asarray(col, np.int64) * a + 128) >> 8


def contour(m):
    """Set pixels with a 4-neighbour that is unset or outside the image: the mask minus the AND of its four shifted copies."""
    p = np.pad(np.asarray(m, bool), 1)
    return p[1:-1, 1:-1] & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def round_corners(v):
    q = np.floor(np.asarray(v, np.float32) + np.float32(0.5)).astype(np.float64)
    q = np.where(np.isnan(q), COORD_MIN, q)
    return np.clip(q, COORD_MIN, COORD_MAX).astype(np.int64)


def outline(H, W, x0, y0, x1, y1, t):
    """The rectangle with inclusive corners minus the rectangle shrunk by t on every side."""
    yy, xx = np.mgrid[0:H, 0:W]
    outer = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
    inner = (xx >= x0 + t) & (xx <= x1 - t) & (yy >= y0 + t) & (yy <= y1 - t)
    return outer & ~inner


def segment(H, W, ax, ay, bx, by, t):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    dx, dy = np.int64(bx - ax), np.int64(by - ay)
    L = dx * dx + dy * dy
    wx, wy = xx - ax, yy - ay
    s = wx * dx + wy * dy
    t2 = np.int64(t) * np.int64(t)
    near_a = 4 * (wx * wx + wy * wy) <= t2
    near_b = 4 * ((xx - bx) ** 2 + (yy - by) ** 2) <= t2
    cross = wx * dy - wy * dx
    band = 4 * cross * cross <= t2 * L
    return np.where((L == 0) | (s <= 0), near_a, np.where(s >= L, near_b, band))


def disc(H, W, kx, ky, r):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    return (xx - kx) ** 2 + (yy - ky) ** 2 <= np.int64(r) * np.int64(r)


def paste(H, W, x0, y0, cells):
    """A boolean block with its top-left at (x0, y0), clipped to the image."""
    on = np.zeros((H, W), bool)
    h, w = cells.shape
    ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
    if ya < yb and xa < xb:
        on[ya:yb, xa:xb] = cells[ya - y0:yb - y0, xa - x0:xb - x0]
    return on


def glyph(H, W, x0, y0, g, scale, font):
    if font is not None and 0 <= g < len(font):
        bits = int(font[g])
        cells = np.array([[(bits >> (5 * r + c)) & 1 for c in range(5)] for r in range(7)], bool)
    else:
        cells = np.ones((7, 5), bool)
    return paste(H, W, x0, y0, np.kron(cells, np.ones((scale, scale), bool)))


def unpack_rgb(rgb):
    return np.array([rgb & 0xFF, (rgb >> 8) & 0xFF, (rgb >> 16) & 0xFF], np.int64)


def check_prim(q):
    two = q['kind'] in (RECT, SEGMENT, FILL)
    ok = 0 <= q['kind'] <= FILL and 0 <= q['a'] <= 256 and 0 <= q['rgb'] <= 0xFFFFFF
    ok = ok and all(COORD_MIN <= q[k] <= COORD_MAX for k in (('x0', 'y0', 'x1', 'y1') if two else ('x0', 'y0')))
    lo = 0 if q['kind'] in (DISC, FILL) else 1
    ok = ok and lo <= q['p'] <= (GLYPH_SCALE_MAX if q['kind'] == GLYPH else PARAM_MAX)
    if not ok:
        raise ValueError('primitive %r breaks a cap' % (q,))


def coverage(H, W, q, font):
    if q['kind'] == RECT:
        return outline(H, W, q['x0'], q['y0'], q['x1'], q['y1'], q['p'])
    if q['kind'] == SEGMENT:
        return segment(H, W, q['x0'], q['y0'], q['x1'], q['y1'], q['p'])
    if q['kind'] == DISC:
        return disc(H, W, q['x0'], q['y0'], q['p'])
    if q['kind'] == GLYPH:
        return glyph(H, W, q['x0'], q['y0'], q['x1'], q['p'], font)
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx >= q['x0']) & (xx <= q['x1']) & (yy >= q['y0']) & (yy <= q['y1'])


def prim_rows(prims):
    """Primitives (a structured array with FIELDS or (P,8) ints) as dicts of Python ints."""
    if prims is None or len(prims) == 0:
        return []
    p = np.asarray(prims)
    if p.dtype.names:
        return [{k: int(r[k]) for k in FIELDS} for r in p]
    return [dict(zip(FIELDS, (int(v) for v in r))) for r in p.reshape(-1, 8)]


def render(img, masks=None, bbox=None, colors=None, order=None, mask_a256=128, box_thickness=1, flags=0, prims=None, font=None):
    img = np.asarray(img, np.float32)
    _, H, W = img.shape
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError('image larger than %d a side' % MAX_SIDE)
    c = round_image(img)
    D = 0 if colors is None else len(colors)
    for d in (range(D) if order is None else [int(o) for o in order]):
        col = np.asarray(colors[d], np.int64)
        if flags & (DRAW_MASKS | DRAW_CONTOURS):
            m = np.asarray(masks[d]) != 0
            if flags & DRAW_MASKS:
                c = np.where(m[:, :, None], blend(c, col, mask_a256), c)
            if flags & DRAW_CONTOURS:
                c = np.where(contour(m)[:, :, None], col, c)
        if flags & DRAW_BOXES:
            top, left, bottom, right = (int(v) for v in round_corners(bbox[d]))
            c = np.where(outline(H, W, left, top, right, bottom, box_thickness)[:, :, None], col, c)
    for q in prim_rows(prims):
        check_prim(q)
        c = np.where(coverage(H, W, q, font)[:, :, None], blend(c, unpack_rgb(q['rgb']), q['a']), c)
    return c.astype(np.uint8)
