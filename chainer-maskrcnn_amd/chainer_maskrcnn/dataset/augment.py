"""Training augmentation: random horizontal flip and scale jitter.  Off unless a ``BatchLoader`` is given an
``Augment``; with it off every transform and loader path is the unaugmented one.

Conventions (the augmented example is ``Transform(hflip(example))`` with the drawn ``min_size``; ``max_size`` is unchanged):
  decisions   (flip, min_size) of an example are a pure function of (seed, rank, ticket) - ticket = the example's position in the
              rank's sequence (``BatchLoader`` numbering) - drawn from a generator seeded with exactly those three numbers: they do not
              depend on the number of loader threads, their timing, or the global ``np.random``.  flip with probability p, min_size
              uniform over the listed sizes.
  flip        in source coordinates, before the resize, for a source of width W:
                image, masks  column i -> W - 1 - i
                boxes         (y1, x1, y2, x2) -> (y1, W - x2, y2, W - x1)       (continuous, chainercv.transforms.flip_bbox)
                keypoints     (x, y, v) with v > 0: x -> W - 1 - x (pixel indices, Detectron's flip_keypoints); v == 0 entries keep
                              their coordinates; then the channels are permuted by the flip map (left <-> right).
  LSJ         large-scale jitter (``Augment(lsj_size=S)``): after the flip the example is resized VIRTUALLY by a random
              factor (``lsj_geometry``: to oh x ow, the longer side S * s, s uniform in ``lsj_scale``) and the window of rows
              y0 .. y0+ch-1, columns x0 .. x0+cw-1 of that resize, at most S x S, lands at the top-left of an S x S canvas; the rest is
              zero.  scale = oh / H as ever, the example's size is (ch, cw).  Mask instances whose cropped mask has no pixel left are
              dropped and the others get the tight box (ymin, xmin, ymax + 1, xmax + 1) of their cropped mask; keypoint instances get
              their box shifted and clipped to the window (dropped when nothing is left), keypoints outside the window get v = 0.
  Copy-Paste  Simple Copy-Paste (``Augment(copy_paste_prob=P)``, on top of LSJ, mask examples, batches of N >= 2): after
              flip and LSJ example n of a batch receives from its partner p = (n + 1) % N.  ``decide_copy_paste`` draws, from a stream
              of its own, whether the example receives (as a target) and which of its annotated instances it offers (as a source, keyed
              by the original instance index, before any crop).  ``AugmentParams.copy_paste`` carries (seed, rank, ticket, P); the
              transform, which knows the raw instance count, calls ``decide_copy_paste`` with it.  ``copy_paste_batch`` is the rule, in
              NumPy: the host path, and the oracle of the device path (csrc/copy_paste.hip).  The partner's offered rows are pasted over
              the image (exact selection, no blending); n's own masks lose the covered pixels, every row gets the tight box of what is
              left of its mask, rows without a pixel are dropped; the survivors come first, then the pasted rows.
  flip map    from the keypoint names: left_* <-> right_* (COCO), *Left <-> *Right (the depth dataset); names without a side map to
              themselves.  A side without its partner is an error: coordinates are never flipped without swapping the channels.
"""
import collections

import numpy as np

# COCO's person keypoints, in the order of the annotation files' person category
COCO_KEYPOINT_NAMES = ('nose', 'left_eye', 'right_eye', 'left_ear', 'right_ear', 'left_shoulder', 'right_shoulder', 'left_elbow',
                       'right_elbow', 'left_wrist', 'right_wrist', 'left_hip', 'right_hip', 'left_knee', 'right_knee', 'left_ankle',
                       'right_ankle')
# the depth dataset's 20 joints, in its joint order (the reference's vis.py get_keypoints)
DEPTH_KEYPOINT_NAMES = ('SpineBase', 'SpineMid', 'Neck', 'Head', 'ShoulderLeft', 'ElbowLeft', 'WristLeft', 'HandLeft', 'ShoulderRight',
                        'ElbowRight', 'WristRight', 'HandRight', 'HipLeft', 'KneeLeft', 'AnkleLeft', 'FootLeft', 'HipRight', 'KneeRight',
                        'AnkleRight', 'FootRight')

# per-example parameters a transform takes: flip (bool), min_size (int or None = the transform's own), keypoint_perm (flip map or None),
# lsj (None, or (S, s, u_y, u_x): canvas size and the three draws of decide_lsj - the geometry follows from the source size, lsj_geometry),
# copy_paste (None, or (seed, rank, ticket, prob): the arguments of decide_copy_paste but the instance count, which the transform knows)
AugmentParams = collections.namedtuple('AugmentParams', ['flip', 'min_size', 'keypoint_perm', 'lsj', 'copy_paste'])
AugmentParams.__new__.__defaults__ = (None, None, None)


def _partner(name):
    for a, b in (('left_', 'right_'), ('right_', 'left_')):
        if name.startswith(a):
            return b + name[len(a):]
    for a, b in (('Left', 'Right'), ('Right', 'Left')):
        if name.endswith(a):
            return name[:-len(a)] + b
    return None


def flip_permutation(names):
    """perm[k] = the channel keypoint k lands in when the image is mirrored (an involution).  Raises ValueError when a left / right name
    has no partner in the list, a name repeats, or the list has no left / right pair at all."""
    names = list(names)
    if len(set(names)) != len(names):
        raise ValueError('keypoint names repeat: %r' % (names,))
    index = {n: k for k, n in enumerate(names)}
    perm, pairs = [], 0
    for k, n in enumerate(names):
        p = _partner(n)
        if p is None:
            perm.append(k)
            continue
        if p not in index:
            raise ValueError('keypoint %r has no mirror partner %r among the keypoint names' % (n, p))
        perm.append(index[p])
        pairs += 1
    if pairs == 0:
        raise ValueError('the keypoint names %r carry no left / right pairing' % (names,))
    return np.array(perm, np.int64)


def decide(seed, rank, ticket, p, min_sizes=None):
    """(flip, min_size) of the example at ``ticket`` of ``rank``'s sequence: a pure function of its arguments."""
    rng = np.random.default_rng([int(seed), int(rank), int(ticket)])
    flip = bool(rng.random() < p)
    min_size = int(min_sizes[int(rng.integers(len(min_sizes)))]) if min_sizes else None
    return flip, min_size


def decide_lsj(seed, rank, ticket, p, scale_range):
    """(flip, s, u_y, u_x) of the example at ``ticket`` of ``rank``'s sequence under large-scale jitter: a pure function of its arguments.
    The first draw is ``decide``'s flip draw; then s uniform in [lo, hi] and the window position u_y, u_x uniform in [0, 1)."""
    lo, hi = float(scale_range[0]), float(scale_range[1])
    rng = np.random.default_rng([int(seed), int(rank), int(ticket)])
    flip = bool(rng.random() < p)
    s = lo + (hi - lo) * float(rng.random())
    return flip, s, float(rng.random()), float(rng.random())


def decide_copy_paste(seed, rank, ticket, prob, n_inst):
    """(receive, sel) of the example at ``ticket`` of ``rank``'s sequence under Copy-Paste: a pure function of its arguments, drawn from
    a stream of its own (``decide`` / ``decide_lsj`` draw from [seed, rank, ticket]).  receive: the example, as a target, takes its
    partner's offer (the first draw < prob); sel (n_inst,) bool: which of its annotated instances it offers as a source (one draw each,
    < 0.5), by original instance index."""
    rng = np.random.default_rng([int(seed), int(rank), int(ticket), 1])
    receive = bool(rng.random() < prob)
    return receive, rng.random(int(n_inst)) < 0.5


def copy_paste_batch(batch, receive, offers, max_gt=None):
    """Simple Copy-Paste on a collated canvas batch (``loader.collate(canvas=S)`` of LSJ'd mask examples): a new batch, the given one is
    only read.  receive (N,): is example n a target; offers: per example, which of its batch rows it offers as a source (bool per row, in
    row order; missing entries count as not offered).  Example n's partner is p = (n + 1) % N.
      pick    the partner's valid rows (label >= 0) that are offered when receive[n], else none; alpha = OR of masks[p, j] != 0 over pick
      image   where(alpha, imgs[p], imgs[n])
      rows    n's valid rows as mask & ~alpha with their labels, then the picked rows unchanged with the partner's labels; those with a
              pixel left, in that order, are packed first with the tight box of their mask (``tight_boxes``); the first G_out stay
      G_out   max_gt, or the largest number of kept rows in the batch (at least 1); behind the kept rows: label -1, zero box, zero plane
      sizes   the elementwise max of n's and p's when receive[n]; scales are unchanged"""
    imgs, masks, labels = np.asarray(batch['imgs']), np.asarray(batch['masks']), np.asarray(batch['labels'])
    N, G = labels.shape
    if N < 2:
        raise ValueError('copy_paste_batch: a batch of at least 2 examples expected (an example receives from its neighbour), got %d' % N)
    rows, out_imgs = [], imgs.copy()
    sizes = np.array(batch['sizes'], copy=True)
    for n in range(N):
        p = (n + 1) % N
        offer = np.zeros((G,), bool)
        o = np.asarray(offers[p], bool).reshape(-1)[:G]
        offer[:len(o)] = o
        pick = np.flatnonzero((labels[p] >= 0) & offer) if receive[n] else np.zeros((0,), np.int64)
        alpha = (masks[p, pick] != 0).any(0) if len(pick) else np.zeros(masks.shape[2:], bool)
        out_imgs[n] = np.where(alpha, imgs[p], imgs[n])
        own = np.flatnonzero(labels[n] >= 0)
        cand = np.concatenate([np.where(alpha, 0, masks[n, own]).astype(masks.dtype), masks[p, pick]])
        boxes, keep = tight_boxes(cand)
        rows.append((cand[keep], boxes[keep], np.concatenate([labels[n, own], labels[p, pick]])[keep]))
        if receive[n]:
            sizes[n] = np.maximum(batch['sizes'][n], batch['sizes'][p])
    G_out = max_gt or max(1, max(len(r[2]) for r in rows))
    out = dict(batch)
    out.update(imgs=out_imgs, sizes=sizes, masks=np.zeros((N, G_out) + masks.shape[2:], masks.dtype),
               bboxes=np.zeros((N, G_out, 4), np.float32), labels=np.full((N, G_out), -1, np.int32))
    for n, (m, b, l) in enumerate(rows):
        g = min(G_out, len(l))
        out['masks'][n, :g], out['bboxes'][n, :g], out['labels'][n, :g] = m[:g], b[:g], l[:g]
    return out


def lsj_geometry(H, W, S, s, u_y, u_x):
    """(oh, ow, y0, x0, ch, cw): an H x W source is resized virtually to oh x ow (its longer side to S * s) and the ch x cw window at
    (y0, x0) of that resize, at most S x S, is what the example keeps."""
    r = min(S * s / H, S * s / W)
    oh, ow = max(1, int(H * r + 0.5)), max(1, int(W * r + 0.5))
    ch, cw = min(oh, S), min(ow, S)
    y0, x0 = min(int(u_y * (oh - ch + 1)), oh - ch), min(int(u_x * (ow - cw + 1)), ow - cw)
    return oh, ow, y0, x0, ch, cw


def tight_boxes(masks):
    """(G,h,w) masks -> ((G,4) float32 boxes (ymin, xmin, ymax + 1, xmax + 1) of the non-zero pixels, (G,) bool: has a pixel).  The box of
    an empty mask is zero."""
    masks = np.asarray(masks)
    boxes = np.zeros((masks.shape[0], 4), np.float32)
    keep = np.zeros((masks.shape[0],), bool)
    for g, m in enumerate(masks):
        ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        if len(ys):
            boxes[g], keep[g] = (ys[0], xs[0], ys[-1] + 1, xs[-1] + 1), True
    return boxes, keep


def crop_boxes_keypoints(bbox, kp, y0, x0, ch, cw):
    """The LSJ rule of keypoint examples, on resized coordinates: bbox (G,4) (y1,x1,y2,x2) and kp (G,K,(y,x,v)) shifted by (-y0, -x0), the
    boxes clipped to [0, ch] x [0, cw]; instances whose clipped box has no height or width are dropped; a keypoint with v > 0 outside
    [0, ch) x [0, cw) gets v = 0 and keeps its shifted coordinates.  Returns (bbox, kp, keep (G,) bool) of the kept rows."""
    bbox = np.array(bbox, np.float32).reshape(-1, 4) - np.array([y0, x0, y0, x0], np.float32)
    bbox[:, 0::2] = np.clip(bbox[:, 0::2], 0, ch)
    bbox[:, 1::2] = np.clip(bbox[:, 1::2], 0, cw)
    keep = (bbox[:, 2] - bbox[:, 0] > 0) & (bbox[:, 3] - bbox[:, 1] > 0)
    kp = np.array(kp, np.float32)
    kp[:, :, 0] -= np.float32(y0)
    kp[:, :, 1] -= np.float32(x0)
    inside = (kp[:, :, 0] >= 0) & (kp[:, :, 0] < ch) & (kp[:, :, 1] >= 0) & (kp[:, :, 1] < cw)
    kp[:, :, 2] = np.where((kp[:, :, 2] > 0) & ~inside, 0, kp[:, :, 2])
    return bbox[keep], kp[keep], keep


def flip_bbox(bbox, W):
    """(G,4) (y1,x1,y2,x2) boxes of a source of width W, mirrored: x1' = W - x2, x2' = W - x1 (a new array)."""
    bbox = np.array(bbox, copy=True).reshape(-1, 4)
    x1 = bbox[:, 1].copy()
    bbox[:, 1] = W - bbox[:, 3]
    bbox[:, 3] = W - x1
    return bbox


def flip_keypoints(keypoints, W, perm):
    """(G,K,3) (x,y,v) keypoints of a source of width W, mirrored: x' = W - 1 - x where v > 0, then channel k moves to perm[k]
    (a new array)."""
    if perm is None:
        raise ValueError('flipping keypoints needs a flip map (left / right channel permutation)')
    kp = np.array(keypoints, copy=True)
    perm = np.asarray(perm)
    if kp.ndim != 3 or kp.shape[1] != len(perm):
        raise ValueError('keypoints (G,%d,3) expected for a flip map of %d names, got %s' % (len(perm), len(perm), kp.shape))
    vis = kp[:, :, 2] > 0
    kp[:, :, 0] = np.where(vis, W - 1 - kp[:, :, 0], kp[:, :, 0])
    out = np.empty_like(kp)
    out[:, perm] = kp
    return out


def hflip(example, keypoint_perm=None):
    """A dataset example mirrored in source coordinates: (img (C,H,W), bbox, label, masks list) of COCOMaskLoader, or (img, bbox,
    keypoints (G,K,(x,y,v))) of COCOKeypointsLoader / DepthDataset (keypoint_perm required)."""
    img = example[0]
    W = img.shape[2]
    out_img = np.ascontiguousarray(img[:, :, ::-1])
    bbox = flip_bbox(example[1], W)
    if len(example) == 4:
        masks = [np.ascontiguousarray(np.asarray(m)[:, ::-1]) for m in example[3]]
        return out_img, bbox, example[2], masks
    if len(example) == 3:
        return out_img, bbox, flip_keypoints(example[2], W, keypoint_perm)
    raise ValueError('hflip: a mask example (4 items) or a keypoint example (3 items) expected, got %d items' % len(example))


class Augment(object):
    """The augmentation of a training run: flip probability, the short sides to draw from (None: the transform's own min_size), the
    seed, and for keypoint data the flip map; ``lsj_size`` = S turns large-scale jitter on (an S x S canvas, the scale drawn from
    ``lsj_scale``; not together with min_sizes - two different resize rules); ``copy_paste_prob`` = P in (0, 1] turns Copy-Paste on (with
    lsj_size only; 0 = off).  ``params(rank, ticket)`` gives an example's AugmentParams."""

    def __init__(self, hflip_prob=0.0, min_sizes=None, seed=0, keypoint_perm=None, lsj_size=None, lsj_scale=(0.1, 2.0),
                 copy_paste_prob=0.0):
        if not 0.0 <= float(hflip_prob) <= 1.0:
            raise ValueError('hflip_prob must lie in [0, 1], got %r' % hflip_prob)
        if min_sizes is not None:
            min_sizes = [int(s) for s in min_sizes]
            if not min_sizes or any(s <= 0 for s in min_sizes):
                raise ValueError('min_sizes must be a non-empty list of positive sizes, got %r' % (min_sizes,))
        self.hflip_prob, self.min_sizes, self.seed = float(hflip_prob), min_sizes, int(seed)
        self.keypoint_perm = None if keypoint_perm is None else np.asarray(keypoint_perm, np.int64)
        self.lsj_size, self.lsj_scale = None, (float(lsj_scale[0]), float(lsj_scale[1]))
        if lsj_size:
            if min_sizes is not None:
                raise ValueError('min_sizes and lsj_size are two different resize rules: give one of them')
            if int(lsj_size) <= 0 or int(lsj_size) % 64:
                raise ValueError('lsj_size must be a positive multiple of 64, got %r' % (lsj_size,))
            if not 0 < self.lsj_scale[0] <= self.lsj_scale[1]:
                raise ValueError('lsj_scale must be 0 < lo <= hi, got %r' % (lsj_scale,))
            self.lsj_size = int(lsj_size)
        self.copy_paste_prob = 0.0
        if copy_paste_prob:
            if not 0.0 < float(copy_paste_prob) <= 1.0:
                raise ValueError('copy_paste_prob must lie in (0, 1] (0 = off), got %r' % (copy_paste_prob,))
            if not self.lsj_size:
                raise ValueError('copy_paste_prob needs lsj_size: Copy-Paste composes two large-scale-jittered canvases')
            if keypoint_perm is not None:
                raise ValueError('copy_paste_prob: Copy-Paste is defined for mask examples, not for keypoint data')
            self.copy_paste_prob = float(copy_paste_prob)

    def params(self, rank, ticket):
        if self.lsj_size:
            flip, s, u_y, u_x = decide_lsj(self.seed, rank, ticket, self.hflip_prob, self.lsj_scale)
            cp = (self.seed, int(rank), int(ticket), self.copy_paste_prob) if self.copy_paste_prob else None
            return AugmentParams(flip, None, self.keypoint_perm, (self.lsj_size, s, u_y, u_x), cp)
        flip, min_size = decide(self.seed, rank, ticket, self.hflip_prob, self.min_sizes)
        return AugmentParams(flip, min_size, self.keypoint_perm)
