"""Edge cases of the proposal, anchor and RoI samplers (csrc/sort.hip, the proposal chain of csrc/rpn.hip, csrc/targets.hip) as pure-NumPy
builders: every builder returns the inputs of one device call and the outputs the oracle (oracle/proposal.py, oracle/targets.py,
oracle/boxes.py) gives for them.  No GPU import: tests/test_sampler_cases_cpu.py asserts from the oracle alone that each case sits
on the edge it is named for; tests/test_rpn_gpu.py and tests/test_targets_gpu.py compare the kernels with the same dictionaries.

Two rules of the device code have no statement in the reference (which raises or is never called there) and are restated here once:
  * an image without objects (n_gt = 0), anchor targets: every anchor inside the image is background, the 256 with the smallest
    (key, index) survive, loc is all zero (k_at_label / k_at_loc of targets.hip);
  * an image without objects, proposal targets: every proposal is a background candidate (max IoU 0), no row is foreground,
    gt_assign = -1, gt_roi_loc = 0, labels 0 (k_proposal_target)."""
import functools

import numpy as np

from oracle import boxes as ob
from oracle import targets as ot
from oracle.proposal import ProposalCreator

F = np.float32
SMALL_FEAT, SMALL_IMG = [(40, 48), (20, 24), (10, 12), (5, 6), (3, 3)], (160, 192)            # A = 7,677
BIG_FEAT, BIG_IMG = [(72, 80), (36, 40), (18, 20), (9, 10), (5, 5)], (288, 320)                 # A = 23,025
AT_FEAT, AT_IMG = [(48, 64), (24, 32), (12, 16), (6, 8), (3, 4)], (192, 256)                    # A = 12,276
RUN = 2048                  # sort.hip: keys per sorted run of the two-launch sort
COMPACT_TRIP = 256 * 2048   # sort.hip: keys one trip of k_compact_ge's tile loop covers (256 workgroups x 2048 keys)


def sort_np(n_pre):
    """The power of two the device sort runs over (top_k_sorted: 64 at the least)."""
    p = 64
    while p < n_pre:
        p <<= 1
    return p


# ======================================================================================================================
# A. top-k selection and sort, through rpn_proposals
# ======================================================================================================================
def _rpn_inputs(seed, N, anchors):
    """The bit-exact convention of tests/test_rpn_gpu.py: dh = dw = 0, standard-normal scores with a run of tied ones."""
    rs = np.random.RandomState(seed)
    A = anchors.shape[0]
    locs = (rs.standard_normal((N, A, 4)) * 0.3).astype(F)
    locs[:, :, 2:] = 0
    scores = rs.standard_normal((N, A, 2)).astype(F)
    if A > 40:
        scores[:, 5:40, 1] = scores[0, 5, 1]
    return locs, scores


def rpn_valid(locs_i, anchors, img_size, min_size):
    """The oracle's min-size filter (oracle/proposal.py) as a mask over the anchors of one image."""
    roi = ob.loc2bbox(anchors, locs_i)
    roi[:, 0::2] = np.clip(roi[:, 0::2], 0, img_size[0])
    roi[:, 1::2] = np.clip(roi[:, 1::2], 0, img_size[1])
    return ((roi[:, 2] - roi[:, 0]) >= F(min_size)) & ((roi[:, 3] - roi[:, 1]) >= F(min_size))


def _rpn_finish(anchors, locs, scores, img_size, min_size, n_pre, n_post, per_image=None, name=''):
    """Adds the oracle's outputs per image: pre_nms_index, nms_keep, rois, levels.  per_image (N,3) = (h, w, min_size) of each image."""
    N, A = locs.shape[:2]
    n_eff = min(n_pre, A)                  # the entry point clamps n_pre to A
    want = []
    for i in range(N):
        size, ms = (img_size, min_size) if per_image is None else ((float(per_image[i, 0]), float(per_image[i, 1])), float(per_image[i, 2]))
        pc = ProposalCreator(n_train_pre_nms=n_eff, n_train_post_nms=n_post, min_size=ms)
        rois, dbg = pc(locs[i], scores[i, :, 1], anchors, size, return_debug=True)
        want.append(dict(pre_nms_index=dbg['pre_nms_index'].astype(np.int64), nms_keep=dbg['nms_keep'], rois=rois,
                         levels=ob.map_rois_to_fpn_levels(rois), n_valid=int(rpn_valid(locs[i], anchors, size, ms).sum())))
    return dict(name=name, anchors=anchors, locs=locs, scores=scores, img_size=img_size, min_size=min_size, n_pre=n_pre, n_eff=n_eff,
                n_post=n_post, per_image=None if per_image is None else np.ascontiguousarray(per_image, F), want=want)


SORT_SHAPES = [1, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 4096, 4097, 6000, 8192, 8193]


@functools.lru_cache(maxsize=None)
def rpn_sort_shape(n_pre):
    """A.1: every shape of the sort; the larger pyramid where n_pre > 4096.  N = 2."""
    big = n_pre > 4096
    anchors = ob.fpn_anchors(BIG_FEAT if big else SMALL_FEAT)
    locs, scores = _rpn_inputs(1, 2, anchors)
    n_post = max(1, min(300, n_pre // 2))
    return _rpn_finish(anchors, locs, scores, BIG_IMG if big else SMALL_IMG, 16.0, n_pre, n_post, name='sort_shape_%d' % n_pre)


@functools.lru_cache(maxsize=None)
def rpn_mixed_valid(n_pre):
    """A.2: N = 3 on the larger pyramid: image 0 keeps more than 6000 boxes, image 1 between 1 and 2047 (its min_size raised), image 2
    none (min_size above the image)."""
    anchors = ob.fpn_anchors(BIG_FEAT)
    locs, scores = _rpn_inputs(7, 3, anchors)
    per = np.array([[288, 320, 16], [288, 320, 120], [288, 320, 400]], F)
    return _rpn_finish(anchors, locs, scores, BIG_IMG, 16.0, n_pre, 300, per_image=per, name='mixed_valid_%d' % n_pre)


@functools.lru_cache(maxsize=None)
def rpn_fewer_anchors_than_n_pre():
    """A.3: one pyramid level of 5 x 5 positions (stride 32, size 128): A = 75 < n_pre = 2000."""
    anchors = ob.fpn_anchors([(5, 5)], feat_strides=(32,), anchor_sizes=(128,))
    locs, scores = _rpn_inputs(11, 2, anchors)
    return _rpn_finish(anchors, locs, scores, (160, 160), 16.0, 2000, 300, name='A75')


@functools.lru_cache(maxsize=None)
def rpn_second_compaction_trip():
    """A.4: A = 524,288 + 2048 + 37 tiled 20 x 20 boxes; the 300 best scores planted half before row 524,288 and half after it, the very
    last row among them."""
    A = COMPACT_TRIP + 2048 + 37
    i = np.arange(A)
    y, x = (i // 1024) * 4.0, (i % 1024) * 4.0
    anchors = np.stack([y, x, y + 20, x + 20], 1).astype(F)
    rs = np.random.RandomState(21)
    locs = np.zeros((1, A, 4), F)
    locs[0, :, :2] = (rs.standard_normal((A, 2)) * 0.3).astype(F)
    scores = rs.standard_normal((1, A, 2)).astype(F)
    lo = rs.choice(COMPACT_TRIP, 150, replace=False)
    hi = COMPACT_TRIP + rs.choice(A - 1 - COMPACT_TRIP, 149, replace=False)
    planted = np.concatenate([lo, hi, [A - 1]])
    scores[0, planted, 1] = (10 + rs.permutation(300) / 16.0).astype(F)
    c = _rpn_finish(anchors, locs, scores, (2100, 4120), 16.0, 300, 50, name='second_trip')
    c['planted'] = planted
    return c


@functools.lru_cache(maxsize=None)
def rpn_index_only_keys(kind, n_pre):
    """A.5: keys that differ only in the index bits.  kind 'equal': every score of image 0 is one positive value, every score of image 1
    one negative value; kind 'lowbit': three neighbouring bit patterns (0x3F800000 + {0, 1, 2}; negated in image 1)."""
    big = n_pre > 4096
    anchors = ob.fpn_anchors(BIG_FEAT if big else SMALL_FEAT)
    locs, scores = _rpn_inputs(13, 2, anchors)
    A = anchors.shape[0]
    if kind == 'equal':
        scores[0, :, 1], scores[1, :, 1] = 0.75, -0.75
    else:
        rs = np.random.RandomState(14)
        # the best value is rare (3 %, the next 7 %) in either image, so the n_pre best span more than one value
        step = np.stack([rs.choice(3, A, p=[0.9, 0.07, 0.03]), rs.choice(3, A, p=[0.03, 0.07, 0.9])])
        v = (np.uint32(0x3F800000) + step.astype(np.uint32)).view(F)
        scores[0, :, 1], scores[1, :, 1] = v[0], -v[1]
    return _rpn_finish(anchors, locs, scores, BIG_IMG if big else SMALL_IMG, 16.0, n_pre, 300, name='%s_%d' % (kind, n_pre))


SPECIALS = [np.inf, -np.inf, np.finfo(F).max, -np.finfo(F).max, np.finfo(F).tiny, -np.finfo(F).tiny, 1e-45, -1e-45, 1e-40, -1e-40]


@functools.lru_cache(maxsize=None)
def rpn_special_scores():
    """A.6: +-inf, the largest and smallest normal, denormals of both signs and 200 + 200 interleaved +0.0 / -0.0 at known valid indices;
    every other score is negative, so the n_pre = 600 best hold all the zeros and the order among them is the index alone."""
    anchors = ob.fpn_anchors(SMALL_FEAT)
    locs, scores = _rpn_inputs(17, 2, anchors)
    scores[:, :, 1] = -np.abs(scores[:, :, 1]) - F(0.5)
    special = []
    for i in range(2):
        ok = np.where(rpn_valid(locs[i], anchors, SMALL_IMG, 16.0))[0]
        idx = ok[100:100 + 3 * (400 + len(SPECIALS)):3]                   # every third valid anchor
        zeros = np.where(np.arange(400) % 2 == 0, F(0.0), F(-0.0)).astype(F)
        scores[i, idx[:400], 1] = zeros if i == 0 else -zeros            # image 1 starts with -0.0
        scores[i, idx[400:], 1] = np.array(SPECIALS, F)
        special.append(idx)
    c = _rpn_finish(anchors, locs, scores, SMALL_IMG, 16.0, 600, 100, name='special_scores')
    c['special_index'] = special
    return c


# ======================================================================================================================
# B. anchor targets
# ======================================================================================================================
def anchor_inside(anchors, img_size):
    return np.where((anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] <= img_size[0]) & (anchors[:, 3] <= img_size[1]))[0]


def _anchor_image_oracle(bbox, anchors, img_size, keys):
    """(label before sampling, loc, label after sampling) of one image, (A,) / (A,4) / (A,)."""
    A = len(anchors)
    inside = anchor_inside(anchors, img_size)
    if len(bbox) == 0:
        # the device rule for an image without objects (restated: the reference raises on an empty bbox array)
        before = np.full(A, -1, np.int32)
        before[inside] = 0
        comp = (np.asarray(keys, np.uint64)[inside] << np.uint64(31)) | inside.astype(np.uint64)
        after = np.full(A, -1, np.int32)
        after[inside[np.argsort(comp, kind='stable')[:256]]] = 0
        return before, np.zeros((A, 4), F), after
    with np.errstate(invalid='ignore', divide='ignore'):
        ins, a, argmax, _, lab = ot.AnchorTargetCreator().labels_before_sampling(bbox, anchors, img_size)
        before = np.full(A, -1, np.int32)
        before[ins] = lab
        loc, after = ot.anchor_targets_from_keys(bbox, anchors, img_size, keys)
    return before, loc, after


def _anchor_finish(anchors, gt, n_gt, img_size, keys, name=''):
    N = gt.shape[0]
    w = [_anchor_image_oracle(gt[i, :n_gt[i]], anchors, img_size, keys[i]) for i in range(N)]
    return dict(name=name, anchors=np.ascontiguousarray(anchors, F), gt=np.ascontiguousarray(gt, F), n_gt=np.asarray(n_gt, np.int32),
                img_size=img_size, keys=np.ascontiguousarray(keys, np.uint32), label_before=np.stack([x[0] for x in w]),
                loc=np.stack([x[1] for x in w]), label=np.stack([x[2] for x in w]))


def _rand_gt(rs, g, H, W, lo=16, hi=150):
    c = rs.uniform(0.1, 0.9, (g, 2)) * [H, W]
    hw = np.exp(rs.uniform(np.log(lo), np.log(hi), (g, 2)))
    return np.concatenate([np.maximum(c - hw / 2, 0), np.minimum(c + hw / 2, [H, W])], 1).astype(F)


def _keys(rs, shape):
    return rs.randint(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)


def _many_positive_scene(seed, gt_cap=256):
    """Image 0: 200 boxes that ARE inside anchors of the finest level (each positive with IoU 1, its neighbours a stride away with IoU
    0.78): far more than 128 positives.  Image 1: 5 random boxes."""
    rs = np.random.RandomState(seed)
    anchors = ob.fpn_anchors(AT_FEAT)
    inside = anchor_inside(anchors, AT_IMG)
    fine = inside[inside < 48 * 64 * 3]
    gt = np.zeros((2, gt_cap, 4), F)
    gt[0, :200] = anchors[rs.choice(fine, 200, replace=False)]
    gt[1, :5] = _rand_gt(rs, 5, *AT_IMG)
    return rs, anchors, gt, np.array([200, 5], np.int32)


@functools.lru_cache(maxsize=None)
def anchor_many_positives():
    """B.1."""
    rs, anchors, gt, n_gt = _many_positive_scene(31)
    return _anchor_finish(anchors, gt, n_gt, AT_IMG, _keys(rs, (2, len(anchors))), name='many_positives')


@functools.lru_cache(maxsize=None)
def anchor_few_negatives():
    """B.2: a 48 x 64 image: few anchors are inside at all, fewer still are negative."""
    rs = np.random.RandomState(32)
    anchors = ob.fpn_anchors([(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)])
    gt = np.zeros((2, 8, 4), F)
    gt[0, :2] = [[4, 6, 40, 44], [10, 30, 44, 62]]
    gt[1, :1] = [[8, 8, 40, 56]]
    return _anchor_finish(anchors, gt, np.array([2, 1], np.int32), (48, 64), _keys(rs, (2, len(anchors))), name='few_negatives')


@functools.lru_cache(maxsize=None)
def anchor_equal_keys(kind):
    """B.3: all keys 0, all keys 0xFFFFFFFF, or two values only ('two'): the survivors are decided by the anchor index."""
    rs, anchors, gt, n_gt = _many_positive_scene(33)
    gt[1] = gt[0]                       # both images have more candidates than are kept, in both classes
    n_gt[1] = n_gt[0]
    A = len(anchors)
    keys = {'zero': np.zeros((2, A), np.uint32), 'ones': np.full((2, A), 0xFFFFFFFF, np.uint32),
            'two': np.where(rs.randint(0, 2, (2, A)) == 1, np.uint32(0x80000001), np.uint32(7)).astype(np.uint32)}[kind]
    return _anchor_finish(anchors, gt, n_gt, AT_IMG, keys, name='equal_keys_' + kind)


@functools.lru_cache(maxsize=None)
def anchor_empty_beside_objects():
    """B.4: n_gt = [0, 5, 0]."""
    rs = np.random.RandomState(34)
    anchors = ob.fpn_anchors(AT_FEAT)
    gt = np.zeros((3, 8, 4), F)
    gt[1, :5] = _rand_gt(rs, 5, *AT_IMG)
    return _anchor_finish(anchors, gt, np.array([0, 5, 0], np.int32), AT_IMG, _keys(rs, (3, len(anchors))), name='empty_beside_objects')


@functools.lru_cache(maxsize=None)
def anchor_full_gt_cap():
    """B.5: gt_cap = 256 = AT_GCAP with G = 256, 255 and 1: small distinct boxes on a 16 x 16 grid."""
    rs = np.random.RandomState(35)
    anchors = ob.fpn_anchors(AT_FEAT)
    g = np.arange(256)
    y, x = (g // 16) * 11.0 + 2, (g % 16) * 15.0 + 3
    hw = rs.randint(8, 30, (256, 2))
    boxes = np.stack([y, x, np.minimum(y + hw[:, 0], 192), np.minimum(x + hw[:, 1], 256)], 1).astype(F)
    gt = np.zeros((3, 256, 4), F)
    gt[0] = boxes
    gt[1, :255] = boxes[::-1][:255]
    gt[2, :1] = boxes[100:101]
    return _anchor_finish(anchors, gt, np.array([256, 255, 1], np.int32), AT_IMG, _keys(rs, (3, len(anchors))), name='full_gt_cap')


@functools.lru_cache(maxsize=None)
def anchor_ties():
    """B.6: gt 0 and 1 identical; gt 2 equal to an inside anchor; gt 3 and 4 mirror images of each other about the centre of anchor
    `mirror_anchor` (integer coordinates: both IoUs are the same float)."""
    rs = np.random.RandomState(36)
    anchors = ob.fpn_anchors(AT_FEAT)

    def square(py, px):                 # the ratio-1 anchor of the finest level at position (py, px): 32 x 32, integer corners
        return (py * 64 + px) * 3 + 1
    eq, mir = square(10, 12), square(30, 40)
    assert anchors[mir, 2] - anchors[mir, 0] == 32 and anchors[mir, 3] - anchors[mir, 1] == 32
    y0, x0, y1, x1 = anchors[mir]
    gt = np.zeros((2, 8, 4), F)
    gt[0, :5] = [[20, 150, 70, 230], [20, 150, 70, 230], anchors[eq], [y0 - 2, x0 - 9, y1 + 2, x1 - 9], [y0 - 2, x0 + 9, y1 + 2, x1 + 9]]
    gt[1, :3] = _rand_gt(rs, 3, *AT_IMG)
    c = _anchor_finish(anchors, gt, np.array([5, 3], np.int32), AT_IMG, _keys(rs, (2, len(anchors))), name='ties')
    c.update(equal_anchor=eq, mirror_anchor=mir)
    return c


@functools.lru_cache(maxsize=None)
def anchor_zero_area_gt():
    """B.7: a zero-area box beside a normal one: its column of IoUs is all zero, so `ious == gt_max` makes every inside anchor with IoU 0
    to it - all of them - positive."""
    rs = np.random.RandomState(37)
    anchors = ob.fpn_anchors(AT_FEAT)
    gt = np.zeros((2, 8, 4), F)
    gt[0, :2] = [[30, 40, 120, 160], [50, 60, 50, 90]]
    gt[1, :2] = [[50, 60, 50, 90], [30, 40, 120, 160]]
    return _anchor_finish(anchors, gt, np.array([2, 2], np.int32), AT_IMG, _keys(rs, (2, len(anchors))), name='zero_area_gt')


@functools.lru_cache(maxsize=None)
def anchor_border_touch():
    """B.8: A = 12,277 (not a multiple of 64); the last anchor's lower edge is the image's: inside by `<=`."""
    rs = np.random.RandomState(38)
    anchors = np.concatenate([ob.fpn_anchors(AT_FEAT), np.array([[152, 100, 192, 150]], F)])
    gt = np.zeros((2, 8, 4), F)
    gt[0, :3] = np.concatenate([[[150, 98, 192, 152]], _rand_gt(rs, 2, *AT_IMG)])
    gt[1, :2] = _rand_gt(rs, 2, *AT_IMG)
    return _anchor_finish(anchors, gt, np.array([3, 2], np.int32), AT_IMG, _keys(rs, (2, len(anchors))), name='border_touch')


# ======================================================================================================================
# C. proposal targets
# ======================================================================================================================
PT_H, PT_W = 512, 640


def _pt_image_oracle(roi, lev, bbox, label, keys, neg_lo):
    """One image: dict(keep, n_pos, assign (per kept row), n_cand (pos, neg), max_iou, label, loc, levels, roi)."""
    nr, G = len(roi), len(bbox)
    allb = np.concatenate([roi, bbox], 0).astype(F)
    if G == 0:
        # the device rule for an image without objects: max IoU 0 for every proposal, nothing is foreground
        max_iou = np.zeros(nr, F)
        neg = np.where((max_iou < F(0.5)) & (max_iou >= F(neg_lo)))[0]
        comp = (np.asarray(keys, np.uint64) << np.uint64(32)) | np.arange(nr, dtype=np.uint64)
        keep = neg if neg.size <= 256 else np.sort(neg[np.argsort(comp[neg], kind='stable')[:256]])
        S = len(keep)
        return dict(keep=keep, n_pos=0, assign=np.full(S, -1, np.int32), n_cand=(0, int(neg.size)), max_iou=max_iou, label=np.zeros(S, np.int32),
                    loc=np.zeros((S, 4), F), levels=lev[keep].astype(np.int32), roi=allb[keep])
    with np.errstate(invalid='ignore', divide='ignore'):
        keep, n_pos, assign, max_iou = ot.proposal_targets_from_keys(roi, bbox, label, keys, neg_iou_thresh_lo=neg_lo)
        n_cand = (int((max_iou >= F(0.5)).sum()), int(((max_iou < F(0.5)) & (max_iou >= F(neg_lo))).sum()))
        want_label = np.asarray(label)[assign[keep]] + 1
        want_label[n_pos:] = 0
        loc = ob.bbox2loc(allb[keep], bbox[assign[keep]]) / np.array([.1, .1, .2, .2], F)
        levels = np.concatenate([lev, ob.map_rois_to_fpn_levels(bbox)])[keep].astype(np.int32)
    return dict(keep=keep, n_pos=int(n_pos), assign=assign[keep].astype(np.int32), n_cand=n_cand, max_iou=max_iou, label=want_label.astype(np.int32),
                loc=loc.astype(F), levels=levels, roi=allb[keep])


def _pt_finish(rois_l, gts_l, labs_l, roi_cap, gt_cap, keys=None, neg_lo=0.0, seed=0, name='', levels_l=None):
    """rois_l / gts_l / labs_l: per-image arrays; padded to (N, roi_cap, 4) / (N, gt_cap, 4) / (N, gt_cap)."""
    N = len(rois_l)
    rois, lev = np.zeros((N, roi_cap, 4), F), np.zeros((N, roi_cap), F)
    gt, lab = np.zeros((N, gt_cap, 4), F), np.zeros((N, gt_cap), np.int32)
    n_r, n_gt = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for i in range(N):
        r, g = np.asarray(rois_l[i], F).reshape(-1, 4), np.asarray(gts_l[i], F).reshape(-1, 4)
        n_r[i], n_gt[i] = len(r), len(g)
        rois[i, :len(r)], gt[i, :len(g)], lab[i, :len(g)] = r, g, labs_l[i]
        with np.errstate(invalid='ignore', divide='ignore'):
            lev[i, :len(r)] = ob.map_rois_to_fpn_levels(r) if levels_l is None else levels_l[i]
    if keys is None:
        keys = _keys(np.random.RandomState(seed + 1000), (N, roi_cap + gt_cap))
        keys[:, 3:9] = keys[:, 3:4]
    keys = np.ascontiguousarray(keys, np.uint32)
    want = []
    for i in range(N):
        kk = np.concatenate([keys[i, :n_r[i]], keys[i, roi_cap:roi_cap + n_gt[i]]])
        want.append(_pt_image_oracle(rois[i, :n_r[i]], lev[i, :n_r[i]], gt[i, :n_gt[i]], lab[i, :n_gt[i]], kk, neg_lo))
    return dict(name=name, rois=rois, lev=lev, n_r=n_r, gt=gt, lab=lab, n_gt=n_gt, keys=keys, neg_lo=neg_lo, roi_cap=roi_cap, gt_cap=gt_cap, want=want)


def _pt_boxes(rs, n, lo=24, hi=256):
    c = rs.uniform(0.15, 0.85, (n, 2)) * [PT_H, PT_W]
    hw = np.exp(rs.uniform(np.log(lo), np.log(hi), (n, 2)))
    return np.concatenate([np.maximum(c - hw / 2, 0), np.minimum(c + hw / 2, [PT_H, PT_W])], 1).astype(F)


def _pt_rois(rs, gt, n, near=0.5, jitter=12.0):
    """n proposals: a share `near` of them jittered ground-truth boxes, the rest random; every side at least 4 long."""
    k = int(round(n * near)) if len(gt) else 0
    j = gt[rs.randint(0, len(gt), k)] + rs.uniform(-jitter, jitter, (k, 4)) if k else np.zeros((0, 4))
    r = np.concatenate([j, _pt_boxes(rs, n - k, 16, 256)], 0)
    r[:, 0], r[:, 1] = np.clip(r[:, 0], 0, PT_H - 4), np.clip(r[:, 1], 0, PT_W - 4)
    r[:, 2], r[:, 3] = np.clip(r[:, 2], r[:, 0] + 4, PT_H), np.clip(r[:, 3], r[:, 1] + 4, PT_W)
    return r.astype(F)


PT_COUNTS = [1, 63, 64, 65, 1024, 1025, 4095, 4096]


@functools.lru_cache(maxsize=None)
def pt_candidate_count(total):
    """C.1: nr + G = total in both images (k_proposal_target sorts over the next power of two >= total, 64 at the least; PT_CAP = 4096).
    4095 and 4096 use roi_cap = 3840, gt_cap = 256 with G = 255 and 256."""
    rs = np.random.RandomState(100 + total)
    big = total >= 4095
    roi_cap, gt_cap = (3840, 256) if big else (2000, 16)
    G = total - 3840 if big else min(total, 8 if total > 100 else 3)
    rois_l, gts_l, labs_l = [], [], []
    for i in range(2):
        gt = _pt_boxes(rs, G, 12, 200) if big else _pt_boxes(rs, G)
        gts_l.append(gt)
        labs_l.append(rs.randint(0, 80, G))
        rois_l.append(_pt_rois(rs, gt, total - G))
    return _pt_finish(rois_l, gts_l, labs_l, roi_cap, gt_cap, seed=total, name='count_%d' % total)


@functools.lru_cache(maxsize=None)
def pt_no_proposals():
    """C.2: n_rois = 0 in both images: the ground-truth boxes are the only candidates."""
    rs = np.random.RandomState(120)
    gts = [_pt_boxes(rs, 5), _pt_boxes(rs, 3)]
    return _pt_finish([np.zeros((0, 4), F)] * 2, gts, [rs.randint(0, 80, 5), rs.randint(0, 80, 3)], 2000, 16, seed=120, name='no_proposals')


@functools.lru_cache(maxsize=None)
def pt_empty_image_of_two():
    """C.3: n_gt = [4, 0]: the image without objects is the second one, behind the offsets of a normal image."""
    rs = np.random.RandomState(121)
    gt = _pt_boxes(rs, 4)
    rois = [_pt_rois(rs, gt, 300), _pt_rois(rs, gt, 300)]
    return _pt_finish(rois, [gt, np.zeros((0, 4), F)], [rs.randint(0, 80, 4), np.zeros(0, np.int32)], 2000, 16, seed=121, name='empty_image_of_two')


@functools.lru_cache(maxsize=None)
def pt_short_sets():
    """C.4: image 0 has fewer than 64 positives and plenty of negatives (256 rows), image 1 plenty of positives and fewer than 192
    negatives (fewer than 256 rows), image 2 no negative at all."""
    rs = np.random.RandomState(122)
    gts = [_pt_boxes(rs, 3, 40, 120), _pt_boxes(rs, 6, 60, 200), _pt_boxes(rs, 4, 60, 200)]
    rois = [_pt_rois(rs, gts[0], 500, near=0.04, jitter=4.0),
            np.concatenate([_pt_rois(rs, gts[1], 300, near=1.0, jitter=3.0), _pt_rois(rs, gts[1], 60, near=0.0)]),
            _pt_rois(rs, gts[2], 200, near=1.0, jitter=2.0)]
    return _pt_finish(rois, gts, [rs.randint(0, 80, len(g)) for g in gts], 2000, 16, seed=122, name='short_sets')


@functools.lru_cache(maxsize=None)
def pt_equal_keys(kind):
    """C.5: all keys 0, all 0xFFFFFFFF, or equal inside each class ('class': foreground candidates one value, all others another)."""
    rs = np.random.RandomState(123)
    gts = [_pt_boxes(rs, 8), _pt_boxes(rs, 7)]
    rois = [_pt_rois(rs, gts[0], 900), _pt_rois(rs, gts[1], 893)]
    labs = [rs.randint(0, 80, 8), rs.randint(0, 80, 7)]
    roi_cap, gt_cap = 2000, 16
    keys = np.zeros((2, roi_cap + gt_cap), np.uint32)
    if kind == 'ones':
        keys[:] = 0xFFFFFFFF
    elif kind == 'class':
        for i in range(2):
            fg = ob.bbox_iou(np.concatenate([rois[i], gts[i]]), gts[i]).max(1) >= F(0.5)
            k = np.where(fg, np.uint32(0x9E3779B9), np.uint32(5)).astype(np.uint32)
            keys[i, :len(rois[i])], keys[i, roi_cap:roi_cap + len(gts[i])] = k[:len(rois[i])], k[len(rois[i]):]
    return _pt_finish(rois, gts, labs, roi_cap, gt_cap, keys=keys, name='equal_keys_' + kind)


@functools.lru_cache(maxsize=None)
def pt_exact_thresholds(neg_lo):
    """C.6: proposal 0 = [0,0,10,10] against the box [0,0,10,5]: IoU exactly 0.5 (foreground, not background); proposal 1 has IoU 0:
    background at neg_lo = 0, in neither set at neg_lo = 0.1."""
    rs = np.random.RandomState(124)
    gt = np.array([[0, 0, 10, 5], [200, 300, 320, 420]], F)
    filler = _pt_rois(rs, gt[1:], 80)
    rois = [np.concatenate([np.array([[0, 0, 10, 10], [400, 100, 440, 160]], F), filler])] * 2
    return _pt_finish(rois, [gt, gt[::-1].copy()], [np.array([3, 7]), np.array([7, 3])], 2000, 16, neg_lo=neg_lo, seed=124,
                      name='thresholds_neg_lo_%g' % neg_lo)


@functools.lru_cache(maxsize=None)
def pt_degenerate_gt(leading_zero_area):
    """C.7: zero-area ground-truth boxes: as candidates their IoU with a zero-area box is 0/0; NumPy's max / argmax give NaN (the first
    one), and NaN is in neither the foreground nor the background set.  A zero-area proposal rides along."""
    rs = np.random.RandomState(125)
    gt = np.array([[10, 10, 50, 50], [20, 20, 20, 40], [20, 20, 20, 40]], F)
    if leading_zero_area:
        gt = np.concatenate([np.array([[30, 30, 30, 60]], F), gt])
    filler = _pt_rois(rs, gt[gt[:, 2] > gt[:, 0]], 60, jitter=5.0)
    filler[:, 2:] = np.minimum(filler[:, 2:], 120)
    filler[:, :2] = np.minimum(filler[:, :2], filler[:, 2:] - 4)
    rois = np.concatenate([filler[:30], np.array([[20, 20, 20, 40]], F), filler[30:]])
    lev = np.concatenate([ob.map_rois_to_fpn_levels(filler[:30]), [0], ob.map_rois_to_fpn_levels(filler[30:])]).astype(F)
    return _pt_finish([rois, filler], [gt, gt[::-1].copy()], [np.arange(len(gt)) + 1] * 2, 2000, 16, seed=125,
                      name='degenerate_gt_%d' % leading_zero_area, levels_l=[lev, ob.map_rois_to_fpn_levels(filler)])


# ======================================================================================================================
# D. mask and keypoint targets of a batch: the offsets of the second image
# ======================================================================================================================
MK_N, MK_SAMPLE, MK_POS_CAP, MK_GT_CAP, MK_H, MK_W, MK_K = 2, 256, 64, 6, 120, 90, 17
MK_N_POS = [(40, 0), (3, 64)]


@functools.lru_cache(maxsize=None)
def mask_keypoint_batch(n_pos, msz=28, kp_size=56):
    """Every one of the 2 x 256 sampler rows holds a plausible RoI and assignment (a wrong row offset then reads wrong data, not
    nothing); each image has its own masks / keypoints; row 1 of every image with positives is a RoI whose truncated crop is empty
    (int(y1) == int(y0)): the kernel's stated rule is an all-zero mask target."""
    rs = np.random.RandomState(200 + n_pos[0] * 100 + n_pos[1])
    masks = (rs.uniform(0, 1, (MK_N, MK_GT_CAP, MK_H, MK_W)) > 0.5).astype(np.uint8)
    kps = np.concatenate([rs.uniform(0, MK_H, (MK_N, MK_GT_CAP, MK_K, 1)), rs.uniform(0, MK_W, (MK_N, MK_GT_CAP, MK_K, 1)),
                          rs.randint(0, 3, (MK_N, MK_GT_CAP, MK_K, 1))], -1).astype(F)
    R = MK_N * MK_SAMPLE
    y0, x0 = rs.uniform(0, MK_H - 2, R), rs.uniform(0, MK_W - 2, R)
    y1 = np.minimum(y0 + np.exp(rs.uniform(np.log(1.5), np.log(MK_H), R)), MK_H + 3.7)
    x1 = np.minimum(x0 + np.exp(rs.uniform(np.log(1.5), np.log(MK_W), R)), MK_W + 2.2)
    sr = np.stack([y0, x0, y1, x1], 1).astype(F)
    ga = rs.randint(0, MK_GT_CAP, R).astype(np.int32)
    empty_rows = []
    for i in range(MK_N):
        if n_pos[i] > 1:
            sr[i * MK_SAMPLE + 1] = [30.2, 10.0, 30.9, 50.0]
            empty_rows.append(i * MK_SAMPLE + 1)
    want_mask = np.full((MK_N * MK_POS_CAP, msz, msz), -1, np.int32)
    want_kp = np.full((MK_N * MK_POS_CAP, MK_K), -1, np.int32)
    for i in range(MK_N):
        for j in range(n_pos[i]):
            row, slot = i * MK_SAMPLE + j, i * MK_POS_CAP + j
            b = sr[row]
            crop = masks[i, ga[row], max(int(b[0]), 0):min(int(b[2]), MK_H), max(int(b[1]), 0):min(int(b[3]), MK_W)]
            want_mask[slot] = 0 if crop.size == 0 else ot.cv2_resize_linear_u8(crop, (msz, msz)).astype(np.int32)
            # the keypoint transform on a COPY of the gt keypoints (tests/test_targets_gpu.py, oracle/targets.py mutate_gt=False)
            iy0, ix0, iy1, ix1 = [int(v) for v in b]
            k = kps[i, ga[row]].copy()
            k[:, :2] = (k[:, :2] - [iy0, ix0]) / [max(iy1 - iy0, 1), max(ix1 - ix0, 1)] * kp_size
            for q, r in enumerate(k):
                y, x, v = [int(t) for t in r]
                want_kp[slot, q] = y * kp_size + x if (v == 2 and 0 <= y < kp_size and 0 <= x < kp_size) else -1
    return dict(masks=masks, kps=kps, sample_roi=sr, gt_assign=ga, n_pos=np.array(n_pos, np.int32), msz=msz, kp_size=kp_size,
                want_mask=want_mask, want_kp=want_kp, empty_rows=empty_rows)
