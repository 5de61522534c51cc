"""The cases of tests/test_augment_edges_gpu.py: the augmentation kernels (csrc/augment.hip, csrc/copy_paste.hip; DESIGN.md §3.11, §3.17,
§3.18) past one workgroup per plane, one ballot round per example and one pass of picked rows, with the thread maps of the mask-side
kernels restated as plain arithmetic.  Imports without the library or a device; tests/test_augment_edge_cases_cpu.py holds every case
against what it is named for and computes the NumPy results, so a case that misses its path fails there instead of silently weakening the
GPU comparison.

An LSJ batch is a list of (masks (count,H,W) uint8, flip, (oh, ow, y0, x0, ch, cw)) as the kernels see it: the layouts are constructed as
the crop sees them, so for flip = 1 the sources are stored mirrored.  A Copy-Paste case is (batch as loader.collate gives it, gather
(N,G) int32, sel (N,Gin) uint8, receive (N,) uint8)."""
import functools

import numpy as np

from chainer_maskrcnn.dataset.augment import copy_paste_batch, tight_boxes
from chainer_maskrcnn.dataset.transforms import resize_linear, resize_nearest
from tests.copy_paste_data import offers_of, rect

# ---- the thread map of the mask-side kernels: a thread takes CHUNK consecutive bytes of one row, NT threads a block, WAVE candidates a
# ballot round of the two finalize kernels, NT picked rows a pass of k_cp_compose
NT, WAVE, CHUNK = 256, 64, 16
BATCH_MAX = 32                              # MRCNN_RESIZE_BATCH_MAX: descriptors passed by value
# the smallest canvases that leave the single-block regime: 4 full blocks of 32 rows; 6 blocks, the last partly idle, block 1 starting
# inside row 19 (vector rows); the same thread map with byte stores, a ragged 8-byte last chunk and float4 image rows
CANVASES = [(128, 128), (100, 208), (100, 200)]
CANVAS_IDS = ['128x128', '100x208', '100x200']
OLD_CANVASES = [(64, 64), (61, 50)]         # what the older GPU tests run: one block per plane


def wq(W):
    return -(-W // CHUNK)


def threads(H, W):
    return H * wq(W)


def blocks(H, W):
    return -(-threads(H, W) // NT)


def block_start(b, W):
    """(row, chunk) of the first thread of block b."""
    return divmod(b * NT, wq(W))


def block_of(y, x, W):
    return (y * wq(W) + x // CHUNK) // NT


def blocks_of(mask):
    """The blocks that see a non-zero byte of an (H,W) plane."""
    ys, xs = np.nonzero(mask)
    return sorted({block_of(int(y), int(x), mask.shape[1]) for y, x in zip(ys, xs)})


def exits_early(b, W, ch):
    """k_mask_crop_reduce's block-uniform test: every row of block b lies below a window of ch rows."""
    return (b * NT) // wq(W) >= ch


def mask_rows_vectorised(W):
    return W % 16 == 0


def image_rows_vectorised(W):
    return W % 4 == 0


def ballot_round(c):
    return c // WAVE


def pack(arrays):
    """(one uint8 buffer, the byte offset of each array in it)."""
    offs = np.cumsum([0] + [a.nbytes for a in arrays])
    buf = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays]) if arrays else np.zeros((0,), np.uint8)
    return buf, [int(o) for o in offs[:-1]]


def points(H, W, pts, value=1):
    m = np.zeros((H, W), np.uint8)
    for y, x in pts:
        m[y, x] = value
    return m


def _stored(exs, flip):
    return [(np.ascontiguousarray(m[:, :, ::-1]) if flip else m, flip, g) for m, g in exs]


# ---- the NumPy rule of the LSJ mask side ----------------------------------------------------------------------------------------------
def np_crop(batch, labels_in, G):
    """NumPy: the cropped planes of every instance, then boxes, labels, gather table and compacted planes."""
    N = len(batch)
    canvas_planes = []
    bboxes, labels, gather = np.zeros((N, G, 4), np.float32), np.full((N, G), -1, np.int32), np.full((N, G), -1, np.int32)
    for n, (m, flip, (oh, ow, y0, x0, ch, cw)) in enumerate(batch):
        planes = [resize_nearest(p[:, ::-1] if flip else p, (oh, ow))[y0:y0 + ch, x0:x0 + cw] for p in m]
        kept = [g for g, p in enumerate(planes) if p.any()][:G]
        for j, g in enumerate(kept):
            ys, xs = np.nonzero(planes[g])
            bboxes[n, j] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
            labels[n, j], gather[n, j] = labels_in[n, g], g
        canvas_planes.append((planes, kept))
    return bboxes, labels, gather, canvas_planes


def labels_of(batch):
    """labels_in (N,Gin) int32 of an LSJ batch: distinct values, -1 past an example's count."""
    Gin = max(1, max(m.shape[0] for m, _, _ in batch))
    labels_in = np.full((len(batch), Gin), -1, np.int32)
    for n, (m, _, _) in enumerate(batch):
        labels_in[n, :m.shape[0]] = 1000 * (n + 1) + np.arange(m.shape[0])
    return labels_in


def mask_rows(batch, offs):
    """The rows of ops.crop_descs for the masks of an LSJ batch packed at offs (their first 7 entries: the rows of ops.resize_descs)."""
    return [(o, m.shape[1], m.shape[2], g[0], g[1], flip, m.shape[0]) + tuple(g[2:]) for o, (m, flip, g) in zip(offs, batch)]


def image_rows(examples, offs):
    """The same for [(image (H,W,3), flip, geometry)]."""
    return [(o, img.shape[0], img.shape[1], g[0], g[1], flip, 0) + tuple(g[2:]) for o, (img, flip, g) in zip(offs, examples)]


def np_lsj(batch, G, canvas):
    """{'labels_in', 'bboxes', 'labels', 'gather', 'masks' (N,G,H,W), 'kept' (per example: every instance that keeps a pixel)}: tight_boxes
    agrees with np_crop's boxes by construction of both; asserted here once."""
    labels_in = labels_of(batch)
    bboxes, labels, gather, planes = np_crop(batch, labels_in, G)
    masks = np.zeros((len(batch), G) + tuple(canvas), np.uint8)
    kept_all = []
    for n, (ps, kept) in enumerate(planes):
        for j, g in enumerate(kept):
            masks[n, j, :ps[g].shape[0], :ps[g].shape[1]] = ps[g]
        kept_all.append([g for g, p in enumerate(ps) if p.any()])
        tb, keep = tight_boxes(masks[n])
        np.testing.assert_array_equal(tb, bboxes[n])
        assert keep.tolist() == (labels[n] >= 0).tolist()
    return {'labels_in': labels_in, 'bboxes': bboxes, 'labels': labels, 'gather': gather, 'masks': masks, 'kept': kept_all}


# ---- case 1: box extremes in different blocks --------------------------------------------------------------------------------------------
def one_pixel_per_block(H, W):
    pts = []
    for b in range(blocks(H, W)):
        live = min(NT, threads(H, W) - b * NT)
        y, c = divmod(b * NT + (11 * b + 5) % live, wq(W))
        pts.append((y, min(c * CHUNK + (3 * b) % CHUNK, W - 1)))
    return pts


def boundary_pixels(b, H, W):
    """A pixel in the first and one in the last chunk of the row block b starts in - that row is split between blocks b - 1 and b where the
    block starts past chunk 0; where it starts a row, the last chunk of the row above and the first of this one."""
    y, c = block_start(b, W)
    return [(y, 5), (y, W - 2)] if c else [(y - 1, W - 2), (y, 5)]


@functools.lru_cache(maxsize=None)
def extremes_case(canvas, flip):
    """Scale 1 on the whole canvas, then an upscaled random example so that the grid's z extent matters."""
    H, W = canvas
    nb = blocks(H, W)
    inst = [points(H, W, [(0, W - 1), (H - 1, 0)]), points(H, W, [(H - 1, W - 1)], 255), points(H, W, one_pixel_per_block(H, W)),
            points(H, W, boundary_pixels(1, H, W), 2), points(H, W, boundary_pixels(nb - 1, H, W), 128)]
    rs = np.random.RandomState(11)
    other = (rs.rand(3, 45, 70) > 0.98).astype(np.uint8)
    return _stored([(np.stack(inst), (H, W, 0, 0, H, W)), (other, (135, 210, 20, 1, min(H, 115), min(W, 209)))], flip)


# ---- case 2: a window shorter than the canvas --------------------------------------------------------------------------------------------
WINDOW_CASES = {'ch40_128x128': ((128, 128), 40), 'ch20_100x208': ((100, 208), 20)}


@functools.lru_cache(maxsize=None)
def window_case(name, flip):
    """Scale 1; instances given in window coordinates.  ch40: block 1 straddles the window's last row, blocks 2 and 3 lie below it; ch20:
    the last window row is the row blocks 0 and 1 share."""
    if name == 'ch40_128x128':
        H, W, y0, x0, ch, cw = 60, 110, 5, 7, 40, 100
        seen = [(points, [(0, 99), (39, 0)], 255),                       # both extremes, in blocks 0 and 1
                (rect, (45 - y0, 59 - y0), (20 - x0, 40 - x0), 1),       # below the window only: dropped
                (rect, (30, 50), (20, 40), 1),                           # cut at the window's last row
                (rect, (0 - y0, 4 - y0), (30, 60), 1),                   # above the window only: dropped
                (rect, (10, 20), (cw, cw + 2), 1),                       # right of the window only: dropped
                (points, [(39, 99)], 2),                                 # the window's last pixel
                (rect, (33, 36), (50, 70), 128)]                         # block 1 only
    else:
        H, W, y0, x0, ch, cw = 50, 208, 3, 0, 20, 208
        seen = [(points, [(19, 0), (19, 207)], 1),                       # the split row: blocks 0 and 1
                (points, [(19, 150)], 255),                              # block 1 only
                (rect, (20, 40), (10, 200), 1),                          # below the window only: dropped
                (points, [(0, 100), (19, 143)], 2),                      # block 0 only, up to the chunk in front of block 1
                (rect, (15, 30), (130, 160), 128)]                       # cut at the window's last row, in both blocks
    inst = []
    for s in seen:
        if s[0] is points:
            inst.append(points(H, W, [(y + y0, x + x0) for y, x in s[1]], s[2]))
        else:
            inst.append(rect(H, W, (s[1][0] + y0, s[1][1] + y0), (s[2][0] + x0, s[2][1] + x0)) * np.uint8(s[3]))
    return _stored([(np.stack(inst), (H, W, y0, x0, ch, cw))], flip)


# ---- case 3: more than one ballot round ----------------------------------------------------------------------------------------------------
BALLOT_CANVAS = (64, 128)                   # 2 blocks per plane; (3, 130, 64, 128) output planes
BALLOT_GEO = (256, 256, 96, 64, 64, 128)    # 32 x 32 sources upscaled 8x: the window shows source rows 12..19, columns 8..23
BALLOT_DROPPED = [3, 64, 70, 127, 128]      # of the 130 instances of example 0: one in round 0, three in round 1, one in round 2
BALLOT_GS = [130, 100, 65, 64, 63]


@functools.lru_cache(maxsize=None)
def ballot_case(flip):
    a = []
    for g in range(130):
        if g in BALLOT_DROPPED:
            a.append(rect(32, 32, (0, 1), (g % 30, g % 30 + 1)))                      # above the window
        else:
            r0 = 11 if g % 10 == 9 else 12 + g % 7                                    # (11: cut at the window's first row)
            c0 = 8 + (3 * g) % 15
            a.append(rect(32, 32, (r0, r0 + 1), (c0, c0 + 1)))
    b = [rect(32, 32, (25, 30), (g % 20, g % 20 + 3)) for g in range(64)] + [rect(32, 32, (14, 16), (10, 12))]
    return _stored([(np.stack(a), BALLOT_GEO), (np.stack(b), BALLOT_GEO), (np.zeros((0, 32, 32), np.uint8), BALLOT_GEO)], flip)


# ---- case 4: N = 32 descriptors by value ----------------------------------------------------------------------------------------------------
MANY_CANVAS = (16, 32)


def many_geometry(n, crop):
    """(H, W, flip, count, geometry) of example n: every example another one; the crop windows grow past the canvas."""
    H, W = 5 + n % 7, 6 + (3 * n) % 11
    if not crop:
        oh, ow = 3 + n % 14, 5 + (5 * n) % 28
        return H, W, n % 2, n % 4, (oh, ow, 0, 0, oh, ow)
    oh, ow = 6 + n, 10 + 2 * n
    ch, cw = min(oh, MANY_CANVAS[0]), min(ow, MANY_CANVAS[1])
    return H, W, n % 2, n % 4, (oh, ow, (3 * n) % (oh - ch + 1), (5 * n) % (ow - cw + 1), ch, cw)


@functools.lru_cache(maxsize=None)
def many_case(crop, flip):
    """(images [(H,W,3) uint8], LSJ batch) of BATCH_MAX examples; flip inverts every example's mirror bit.  The masks are stored as they
    are (random: nothing is constructed in window coordinates)."""
    rs = np.random.RandomState(5)
    imgs, batch = [], []
    for n in range(BATCH_MAX):
        H, W, f, count, geo = many_geometry(n, crop)
        imgs.append(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
        batch.append(((rs.rand(count, H, W) > 0.6).astype(np.uint8), f ^ flip, geo))
    return imgs, batch


# ---- the image writer -----------------------------------------------------------------------------------------------------------------------
def image_case(canvas, flip):
    """[(image (H,W,3) uint8, flip, geometry)]: upscaled with an interior window, downscaled far below the canvas, scale 1 through a
    window."""
    Hc, Wc = canvas
    rs = np.random.RandomState(3)
    shapes = [((40, 52), (160, 260, 17, 23, Hc, Wc)), ((91, 127), (45, 63, 0, 0, 45, 63)), ((Hc + 9, Wc + 20), (Hc + 9, Wc + 20, 4, 13, Hc, Wc))]
    return [(rs.randint(0, 256, hw + (3,)).astype(np.uint8), (n + flip) % 2, geo) for n, (hw, geo) in enumerate(shapes)]


def np_images(examples, canvas, div=255.0):
    want = np.zeros((len(examples), 3) + tuple(canvas), np.float32)
    for n, (img, flip, (oh, ow, y0, x0, ch, cw)) in enumerate(examples):
        chw = img.transpose(2, 0, 1).astype(np.float32)
        want[n, :, :ch, :cw] = (resize_linear(chw[..., ::-1] if flip else chw, (oh, ow)) / np.float32(div))[:, y0:y0 + ch, x0:x0 + cw]
    return want


# ---- Copy-Paste -------------------------------------------------------------------------------------------------------------------------------
def cp_batch(masks, labels, seed, gather=None, sel=None, receive=None):
    masks, labels = np.ascontiguousarray(masks, np.uint8), np.asarray(labels, np.int32)
    N, G, H, W = masks.shape
    bboxes = np.stack([tight_boxes(m)[0] for m in masks])
    batch = {'imgs': np.random.RandomState(seed).rand(N, 3, H, W).astype(np.float32), 'masks': masks, 'labels': labels, 'bboxes': bboxes,
             'scales': np.ones((N,), np.float32), 'sizes': np.tile(np.array([[H, W]], np.float32), (N, 1))}
    if gather is None:                      # the identity on the valid rows
        gather = np.where(labels >= 0, np.arange(G, dtype=np.int32)[None], -1)
    sel = np.ones((N, G), np.uint8) if sel is None else sel
    receive = np.ones((N,), np.uint8) if receive is None else receive
    return batch, np.ascontiguousarray(gather, np.int32), np.ascontiguousarray(sel, np.uint8), np.ascontiguousarray(receive, np.uint8)


def cp_candidates(case):
    """(N, 2G) int: what becomes of candidate c of example n by the rule - -1 no candidate, 0 dropped (no pixel left), 1 kept.  c < G: own
    row c; c >= G: row c - G of the partner."""
    batch, gather, sel, receive = case
    masks, labels = batch['masks'], batch['labels']
    N, G = labels.shape
    offers = offers_of(gather, sel)
    state = np.full((N, 2 * G), -1, np.int64)
    for n in range(N):
        p = (n + 1) % N
        pick = (labels[p] >= 0) & np.asarray(offers[p], bool) & bool(receive[n])
        alpha = (masks[p, pick] != 0).any(0) if pick.any() else np.zeros(masks.shape[2:], bool)
        for g in range(G):
            if labels[n, g] >= 0:
                state[n, g] = int(np.where(alpha, 0, masks[n, g]).any())
            if pick[g]:
                state[n, G + g] = int(masks[p, g].any())
    return state


def np_copy_paste(case, G_out):
    batch, gather, sel, receive = case
    return copy_paste_batch(batch, receive, offers_of(gather, sel), G_out)


def _random_rect(rs, H, W, x_lo=0):
    y, x = int(rs.randint(0, H - 12)), int(rs.randint(x_lo, W - 12))
    return rect(H, W, (y, y + int(rs.randint(2, 12))), (x, x + int(rs.randint(2, 12))))


# case 5.  Rows of example 0 / its partner, example 1 (label):
#   tall (1)      rows 5..H-6 under the partner's `cover` (5, rows 15..H-16): what is left lies in the first block and in one near the end
#   inside (2)    inside `cover`: dropped
#   corner (3)    the last two rows' last 20 columns under `strip` (6, all of it but the last column): its last pixels are in the last block
#   the rest      random rectangles; row 2 of example 1 (7) is not offered
MULTI_G = 5


@functools.lru_cache(maxsize=None)
def cp_multiblock(canvas, N):
    H, W = canvas
    rs = np.random.RandomState(13 + N)
    zero = np.zeros((H, W), np.uint8)
    ex = [[rect(H, W, (5, H - 6), (40, 60)), rect(H, W, (40, 50), (45, 55)), rect(H, W, (H - 2, H - 1), (W - 20, W - 1)), _random_rect(rs, H, W), zero],
          [rect(H, W, (15, H - 16), (30, 70)), rect(H, W, (H - 2, H - 1), (W - 20, W - 2)), _random_rect(rs, H, W), _random_rect(rs, H, W, 100), zero]]
    labels = [[1, 2, 3, 4, -1], [5, 6, 7, 8, -1]]
    sel = [[1, 0, 0, 1, 1], [1, 1, 0, 1, 1]]
    if N == 3:
        ex.append([_random_rect(rs, H, W), _random_rect(rs, H, W), _random_rect(rs, H, W), zero, zero])
        labels.append([9, 10, 11, -1, -1])
        sel.append([1, 0, 1, 1, 1])
    receive = [1, 1, 0][:N]
    return cp_batch(np.stack([np.stack(e) for e in ex]), labels, 17, sel=np.array(sel, np.uint8), receive=np.array(receive, np.uint8))


# case 6.  128 x 128 in cells of 8 x 8; row g of example n sits in cell 4 ((g + 20 n) % 60) - every fourth cell, over the whole canvas - so
# the partner's row j lies on own rows j + 20 and j - 40.  Three shapes by g % 3 - 4 x 4, its top half, 6 x 6 - so a picked row drops, cuts or only overlaps the row under it.
# gather skips original instance 5 (dropped by the crop); original o is offered where o % 5 == 0.
WAVE_CANVAS = (128, 128)
WAVE_GS = [40, 70]


def _cell_rect(g, cell):
    H, W = WAVE_CANVAS
    cy, cx = 8 * ((cell % 256) // 16), 8 * (cell % 16)
    return [rect(H, W, (cy + 2, cy + 5), (cx + 2, cx + 5)), rect(H, W, (cy + 2, cy + 3), (cx + 2, cx + 5)), rect(H, W, (cy + 1, cy + 6), (cx + 1, cx + 6))][g % 3]


@functools.lru_cache(maxsize=None)
def cp_waves(G):
    N = 3
    valid = [G, G - 4, G - 2]
    masks = np.zeros((N, G) + WAVE_CANVAS, np.uint8)
    labels, gather = np.full((N, G), -1, np.int32), np.full((N, G), -1, np.int32)
    for n in range(N):
        for g in range(valid[n]):
            masks[n, g] = _cell_rect(g, 4 * ((g + 20 * n) % 60))
            labels[n, g], gather[n, g] = 100 * (n + 1) + g, g + (g >= 5)
    sel = np.tile((np.arange(G + 1) % 5 == 0).astype(np.uint8), (N, 1))
    return cp_batch(masks, labels, 19, gather=gather, sel=sel)


def wave_g_outs(G):
    """{kept, 64, 65, 33, > kept}: kept of example 0, and one row past the most any example keeps."""
    kept = (cp_candidates(cp_waves(G)) == 1).sum(1)
    return sorted({int(kept[0]), 64, 65, 33, int(kept.max()) + 1})


# case 7.  G = 257: k_cp_compose stages the picks in two passes, of 256 rows and of 1
MANY_ROWS_G, MANY_ROWS_CANVAS = 257, (16, 48)
MANY_ROWS_PICKS = [[3, 100, 255, 256], [256]]      # what examples 0 and 1 offer
MANY_ROWS_G_OUT = 264                              # room for every kept row


@functools.lru_cache(maxsize=None)
def cp_many_rows():
    G, (H, W) = MANY_ROWS_G, MANY_ROWS_CANVAS
    masks = np.zeros((2, G, H, W), np.uint8)
    for n in range(2):
        for g in range(G):
            y, x = (g + 3 * n) % 15, (7 * g + 5 * n) % 46
            masks[n, g, y:y + 2, x:x + 3] = 1
    masks[0, 200], masks[1, 10] = masks[1, 256], masks[0, 255]          # an own row under a picked one, in either example: dropped
    labels = np.stack([1 + np.arange(G), 1001 + np.arange(G)]).astype(np.int32)
    sel = np.zeros((2, G), np.uint8)
    for n in range(2):
        sel[n, MANY_ROWS_PICKS[n]] = 1
    return cp_batch(masks, labels, 23, sel=sel)


# case 8.  Every byte lane of a word (x % 4) sees 2, 128, 255 and 1 as y varies
BYTE_VALUES = [2, 128, 255, 1]


@functools.lru_cache(maxsize=None)
def cp_byte_values(canvas):
    batch, gather, sel, receive = cp_multiblock(canvas, 3)
    H, W = canvas
    pattern = np.array(BYTE_VALUES, np.uint8)[(np.arange(W)[None] + np.arange(H)[:, None]) % 4]
    return (dict(batch, masks=batch['masks'] * pattern),) + (gather, sel, receive)


# case 10.  Nothing is pasted: no example receives, or no instance is offered.  Row 1 of the last example is valid and empty, so that
# "compacted" moves a row.
@functools.lru_cache(maxsize=None)
def cp_no_paste(kind):
    batch, gather, sel, receive = cp_multiblock((100, 208), 3)
    masks = batch['masks'].copy()
    masks[2, 1] = 0
    batch = dict(batch, masks=masks)
    if kind == 'receive':
        return batch, gather, sel, np.zeros_like(receive)
    return batch, gather, np.zeros_like(sel), np.ones_like(receive)
