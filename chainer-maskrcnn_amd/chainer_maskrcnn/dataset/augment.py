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
# lsj (None, or (S, s, u_y, u_x): canvas size and the three draws of decide_lsj - the geometry follows from the source size, lsj_geometry)
AugmentParams = collections.namedtuple('AugmentParams', ['flip', 'min_size', 'keypoint_perm', 'lsj'])
AugmentParams.__new__.__defaults__ = (None, None)


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
    ``lsj_scale``; not together with min_sizes - two different resize rules).  ``params(rank, ticket)`` gives an example's AugmentParams."""

    def __init__(self, hflip_prob=0.0, min_sizes=None, seed=0, keypoint_perm=None, lsj_size=None, lsj_scale=(0.1, 2.0)):
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

    def params(self, rank, ticket):
        if self.lsj_size:
            flip, s, u_y, u_x = decide_lsj(self.seed, rank, ticket, self.hflip_prob, self.lsj_scale)
            return AugmentParams(flip, None, self.keypoint_perm, (self.lsj_size, s, u_y, u_x))
        flip, min_size = decide(self.seed, rank, ticket, self.hflip_prob, self.min_sizes)
        return AugmentParams(flip, min_size, self.keypoint_perm)
