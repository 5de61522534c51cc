"""The literal statement of Boundary IoU (Cheng et al., "Boundary IoU: Improving Object-Centric Image Segmentation Evaluation", CVPR 2021)
that the boundary tests compare against, written as the published procedure reads: pad the mask by one background pixel, erode d times
with a 3 x 3 block of ones, crop, and keep what the erosion removed.  It shares nothing with evaluations.mask_boundary (cumulative sums) or
with the kernel (packed words, doubling steps)."""
import math

import numpy as np

PINNED_DILATIONS = {(375, 500): 12, (75, 100): 2, (480, 640): 16, (427, 640): 15, (800, 1333): 31, (1024, 1024): 29, (10, 10): 1,
                    (1, 1): 1, (2228, 2228): 63}


def ref_dilation(H, W, ratio=0.02):
    d = int(round(ratio * math.sqrt(H * H + W * W)))
    return 1 if d < 1 else d


def _erode3x3(p):
    """One erosion of the 2-D 0/1 array p by a 3 x 3 block of ones; the array's own border pixels have neighbours outside it, which
    count as background, so they come out 0."""
    out = np.zeros_like(p)
    h, w = p.shape
    acc = np.ones((h - 2, w - 2), dtype=p.dtype)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            acc = acc & p[dy:dy + h - 2, dx:dx + w - 2]
    out[1:h - 1, 1:w - 1] = acc
    return out


def ref_boundary(mask, d):
    """(H, W) any dtype (nonzero = set) -> bool band M & ~E."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), np.uint8)
    p[1:h + 1, 1:w + 1] = m
    for _ in range(d):
        p = _erode3x3(p)
    e = p[1:h + 1, 1:w + 1]
    return (m & (1 - e)).astype(bool)


def ref_boundaries(masks, d):
    masks = np.asarray(masks)
    return np.array([ref_boundary(m, d) for m in masks], dtype=bool).reshape(masks.shape)


def _iou(i, a, g, crowd):
    if i == 0:
        return 0.0
    return float(i) / float(a if crowd else a + g - i)


def ref_pair_iou(dm, gm, d, crowd=False):
    """(mask IoU, boundary IoU, their minimum) of one detection mask and one ground-truth mask, as Python floats from integer counts."""
    dm, gm = np.asarray(dm) != 0, np.asarray(gm) != 0
    db, gb = ref_boundary(dm, d), ref_boundary(gm, d)
    mi = _iou(int((dm & gm).sum()), int(dm.sum()), int(gm.sum()), crowd)
    bi = _iou(int((db & gb).sum()), int(db.sum()), int(gb.sum()), crowd)
    return mi, bi, min(mi, bi)


def ref_boundary_iou_matrix(dts, gts, crowds, d):
    """(D, G) float64 of ref_pair_iou's minimum."""
    o = np.zeros((len(dts), len(gts)))
    for g, gm in enumerate(gts):
        for i, dm in enumerate(dts):
            o[i, g] = ref_pair_iou(dm, gm, d, bool(crowds[g]))[2]
    return o


def ref_counts(a, b, d):
    """Exact (inter, area_a, area_b, binter, barea_a, barea_b) of two mask stacks, int64."""
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    n = int(np.prod(a.shape[1:]))
    A, B = a.reshape(len(a), n).astype(np.int64), b.reshape(len(b), n).astype(np.int64)
    ba, bb = ref_boundaries(a, d).reshape(len(a), n).astype(np.int64), ref_boundaries(b, d).reshape(len(b), n).astype(np.int64)
    return A @ B.T, A.sum(1), B.sum(1), ba @ bb.T, ba.sum(1), bb.sum(1)


def unpack_words(words, W):
    """(D, H, ceil(W/64)) int64 packed rows -> (D, H, W) bool and the tail bits (D, H, 64 * NW - W) (which must be zero)."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint64)
    D, H, NW = w.shape
    bits = np.unpackbits(w.astype('<u8').view(np.uint8).reshape(D, H, NW * 8), axis=-1, bitorder='little')
    return bits[:, :, :W].astype(bool), bits[:, :, W:]


def ref_cocoeval_boundary_iou(dts, gts, iou_type='segm'):
    """Stands in for the IoU of the restated COCOeval (test_coco_eval_cpu._ref_iou, same signature): the (D, G) Boundary IoU of
    dts[i]['mask'] and gts[g]['mask'], d by the rule from the masks' own size."""
    o = np.zeros((len(dts), len(gts)))
    if not len(dts) or not len(gts):
        return o
    d = ref_dilation(*np.asarray(gts[0]['mask']).shape)
    dm, gm = [np.asarray(x['mask']) != 0 for x in dts], [np.asarray(x['mask']) != 0 for x in gts]
    db, gb = [ref_boundary(m, d) for m in dm], [ref_boundary(m, d) for m in gm]
    for g in range(len(gts)):
        crowd = bool(gts[g]['iscrowd'])
        for i in range(len(dts)):
            mi = _iou(int((dm[i] & gm[g]).sum()), int(dm[i].sum()), int(gm[g].sum()), crowd)
            bi = _iou(int((db[i] & gb[g]).sum()), int(db[i].sum()), int(gb[g].sum()), crowd)
            o[i, g] = min(mi, bi)
    return o
