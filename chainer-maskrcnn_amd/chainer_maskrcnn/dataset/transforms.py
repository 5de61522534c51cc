"""Training transforms of the reference (train.py:21-37 ``Transform``, train_keypoints.py:51-68) on the host.

The reference resizes through ChainerCV / OpenCV (``chainercv.transforms.resize`` = ``cv2.resize`` INTER_LINEAR on
float32 when cv2 is importable - train.py:8 imports it - and ``cv2.resize(..., INTER_NEAREST)`` for the masks).
Neither package exists on the target machine, so the two interpolations are restated here in NumPy with OpenCV's
coordinate rules (parity unpinned; the float path is checked against the independent oracle restatement):
  INTER_LINEAR  fx = (dx + 0.5) * (src/dst) - 0.5, sx = floor(fx), clamped to the edge; horizontal pass then vertical
                pass, float32 coefficients
  INTER_NEAREST sx = min(floor(dx * (src/dst)), src - 1)
"""
import numpy as np

from chainer_maskrcnn.dataset.augment import (crop_boxes_keypoints, decide_copy_paste, flip_bbox, flip_keypoints, hflip, lsj_geometry,
                                              tight_boxes)

F = np.float32


def _linear_taps(dst, src):
    scale = 1.0 / (float(dst) / float(src))            # cv2: inv_scale = dsize/ssize (double); scale = 1/inv_scale
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F)).astype(F)
    lo = s < 0
    f[lo], s[lo] = 0, 0
    hi = s >= src - 1
    f[hi], s[hi] = 0, src - 1
    s1 = np.minimum(s + 1, src - 1)
    return s, s1, (F(1) - f).astype(F), f


def resize_linear(img, out_hw):
    """img (C,H,W) float32 -> (C,oh,ow) float32, cv2.resize(..., INTER_LINEAR) per channel."""
    img = np.asarray(img, F)
    C, H, W = img.shape
    oh, ow = out_hw
    if (oh, ow) == (H, W):
        return img.copy()
    x0, x1, a0, a1 = _linear_taps(ow, W)
    y0, y1, b0, b1 = _linear_taps(oh, H)
    rows = img[:, :, x0] * a0 + img[:, :, x1] * a1                  # horizontal pass on every source row
    return (rows[:, y0, :] * b0[:, None] + rows[:, y1, :] * b1[:, None]).astype(F)


def resize_nearest(mask, out_hw):
    """mask (H,W) any dtype -> (oh,ow), cv2.resize(mask, (ow,oh), interpolation=cv2.INTER_NEAREST)."""
    H, W = mask.shape
    oh, ow = out_hw
    sx = np.minimum(np.floor(np.arange(ow) * (1.0 / (float(ow) / W))).astype(np.int64), W - 1)
    sy = np.minimum(np.floor(np.arange(oh) * (1.0 / (float(oh) / H))).astype(np.int64), H - 1)
    return np.ascontiguousarray(mask[sy][:, sx])


def resize_bbox(bbox, in_size, out_size):
    """chainercv.transforms.resize_bbox: (y1,x1,y2,x2) scaled by out/in per axis."""
    bbox = np.array(bbox, dtype=np.float32).reshape(-1, 4)
    ys, xs = float(out_size[0]) / in_size[0], float(out_size[1]) / in_size[1]
    bbox[:, 0] *= ys
    bbox[:, 2] *= ys
    bbox[:, 1] *= xs
    bbox[:, 3] *= xs
    return bbox


def prepare(img, min_size=600, max_size=1000):
    """MaskRCNN.prepare on the host (maskrcnn.py:261-276): short side -> min_size unless the long side would exceed
    max_size; values scaled to [0,1]; no mean subtraction."""
    _, H, W = img.shape
    scale = min_size / min(H, W)
    if scale * max(H, W) > max_size:
        scale = max_size / max(H, W)
    return resize_linear(img, (int(H * scale), int(W * scale))) / F(255)


def _lsj_image(img, aug):
    """Large-scale jitter of an (already mirrored) image (C,H,W): (the ch x cw window of its oh x ow resize, / 255; the geometry)."""
    _, H, W = img.shape
    geo = lsj_geometry(H, W, *aug.lsj)
    oh, ow, y0, x0, ch, cw = geo
    return np.ascontiguousarray((resize_linear(img, (oh, ow)) / F(255))[:, y0:y0 + ch, x0:x0 + cw]), geo


class Transform(object):
    """train.py:21-37.  in: (img, bbox, label, masks list) -> (img, bbox, label, masks (G,oH,oW) uint8, scale).
    aug (dataset.augment.AugmentParams, optional): the example is mirrored first (augment.hflip) when aug.flip, and resized to
    aug.min_size when that is given.  With aug.lsj (large-scale jitter) image and masks are the crop window of the
    mirrored example's virtual resize, instances without a pixel left are dropped and the boxes are the cropped masks' tight boxes.
    With aug.copy_paste (Copy-Paste) two more items follow the scale: receive (bool: the example takes its batch
    partner's offer) and offered (bool per kept row: the row is offered to the example's receiver) - ``augment.decide_copy_paste`` for the
    example's annotated instances, the offer carried through the crop; ``BatchLoader`` applies them after collating."""

    def __init__(self, faster_rcnn):
        self.min_size, self.max_size = faster_rcnn.min_size, faster_rcnn.max_size

    def _lsj(self, in_data, aug):
        img, _, label, label_img = in_data
        H = img.shape[1]
        img, (oh, ow, y0, x0, ch, cw) = _lsj_image(img, aug)
        masks = [resize_nearest(np.asarray(im), (oh, ow))[y0:y0 + ch, x0:x0 + cw] for im in label_img]
        masks = np.stack(masks).astype(np.uint8) if masks else np.zeros((0, ch, cw), np.uint8)
        bbox, keep = tight_boxes(masks)
        out = img, bbox[keep], np.asarray(label, np.int32)[keep], np.ascontiguousarray(masks[keep]), oh / H
        if aug.copy_paste is not None:
            receive, sel = decide_copy_paste(*aug.copy_paste, n_inst=len(keep))
            out += (receive, sel[keep])
        return out

    def __call__(self, in_data, aug=None):
        min_size = self.min_size
        if aug is not None:
            in_data = hflip(in_data) if aug.flip else in_data
            min_size = aug.min_size or min_size
            if aug.lsj is not None:
                return self._lsj(in_data, aug)
        img, bbox, label, label_img = in_data
        _, H, W = img.shape
        img = prepare(img, min_size, self.max_size)
        _, o_H, o_W = img.shape
        scale = o_H / H
        bbox = resize_bbox(bbox, (H, W), (o_H, o_W))
        bbox[:, 2:] = np.maximum(bbox[:, 2:], bbox[:, 2:] + 1)           # == += 1 (train.py:32)
        masks = [resize_nearest(np.asarray(im), (o_H, o_W)) for im in label_img]
        masks = np.stack(masks).astype(np.uint8) if masks else np.zeros((0, o_H, o_W), np.uint8)
        return img, bbox, np.asarray(label, np.int32), masks, scale


class KeypointTransform(object):
    """train_keypoints.py:51-68.  in: (img, bbox, keypoints (G,17,(x,y,v))) -> (img, bbox, label = 0, kp (G,17,(y,x,v)), scale).
    aug: as Transform; a flip needs aug.keypoint_perm.  With aug.lsj the boxes and keypoints follow augment.crop_boxes_keypoints."""

    def __init__(self, faster_rcnn):
        self.min_size, self.max_size = faster_rcnn.min_size, faster_rcnn.max_size

    def _lsj(self, in_data, aug):
        img, bbox, keypoints = in_data
        _, H, W = img.shape
        img, (oh, ow, y0, x0, ch, cw) = _lsj_image(img, aug)
        scale = oh / H
        keypoints = keypoints.astype(np.float32)
        kp = np.concatenate([keypoints[:, :, [1, 0]] * scale, keypoints[:, :, 2, None]], axis=2)
        bbox, kp, _ = crop_boxes_keypoints(resize_bbox(bbox, (H, W), (oh, ow)), kp, y0, x0, ch, cw)
        return img, bbox, np.zeros(bbox.shape[0], dtype=np.int32), kp, scale

    def __call__(self, in_data, aug=None):
        min_size = self.min_size
        if aug is not None:
            in_data = hflip(in_data, aug.keypoint_perm) if aug.flip else in_data
            min_size = aug.min_size or min_size
            if aug.lsj is not None:
                return self._lsj(in_data, aug)
        img, bbox, keypoints = in_data
        _, H, W = img.shape
        img = prepare(img, min_size, self.max_size)
        _, o_H, o_W = img.shape
        scale = o_H / H
        bbox = resize_bbox(bbox, (H, W), (o_H, o_W))
        label = np.zeros(bbox.shape[0], dtype=np.int32)
        keypoints = keypoints.astype(np.float32)
        kp = keypoints[:, :, [1, 0]]
        kp = np.concatenate([kp * scale, keypoints[:, :, 2, None]], axis=2)
        return img, bbox, label, kp, scale


class RawTransform(object):
    """Host half of the device-side Transform: everything except the two resizes, which run on the GPU
    (mrcnn_image_resize_u8_f32 / mrcnn_mask_resize_nearest_u8) on the raw uint8 data.  Returns
    (img_u8 (H,W,3), bbox, label, masks_u8 (G,H,W) | keypoints, scale, (oH,oW)).
    aug (dataset.augment.AugmentParams, optional): (oH,oW) follow aug.min_size when given; with aug.flip the boxes and keypoints are
    mirrored here, while the image and masks stay as decoded - they are mirrored by the batched resize kernels, which read the 7th item
    of the output, the flip flag (returned whenever aug is given).
    With aug.lsj (large-scale jitter) the 6th item is the window size (ch,cw) and an 8th item carries the geometry (oh,ow,y0,x0,ch,cw) of
    augment.lsj_geometry for the crop kernels.  Keypoint examples get their boxes and keypoints here (augment.crop_boxes_keypoints); mask
    examples return bbox = None, every raw mask and label: which instances survive the crop, and their boxes, is decided on the device.
    With aug.copy_paste a mask example carries a 9th item (receive, sel): ``augment.decide_copy_paste`` for its annotated instances, sel
    by original instance index - the device looks the offer of a kept row up through the crop's gather table."""

    def __init__(self, faster_rcnn, keypoints=False):
        self.min_size, self.max_size, self.keypoints = faster_rcnn.min_size, faster_rcnn.max_size, keypoints

    def out_size(self, H, W, min_size=None):
        scale = (min_size or self.min_size) / min(H, W)
        if scale * max(H, W) > self.max_size:
            scale = self.max_size / max(H, W)
        return int(H * scale), int(W * scale)

    def _lsj(self, in_data, aug):
        _, H, W = in_data[0].shape
        flip = bool(aug.flip)
        geo = lsj_geometry(H, W, *aug.lsj)
        oh, ow, y0, x0, ch, cw = geo
        scale = oh / H
        img_u8 = np.ascontiguousarray(in_data[0].transpose(1, 2, 0)).astype(np.uint8)
        if self.keypoints:
            keypoints = (flip_keypoints(in_data[2], W, aug.keypoint_perm) if flip else in_data[2]).astype(np.float32)
            kp = np.concatenate([keypoints[:, :, [1, 0]] * scale, keypoints[:, :, 2, None]], axis=2)
            bbox = resize_bbox(flip_bbox(in_data[1], W) if flip else in_data[1], (H, W), (oh, ow))
            bbox, kp, _ = crop_boxes_keypoints(bbox, kp, y0, x0, ch, cw)
            return img_u8, bbox, np.zeros(bbox.shape[0], dtype=np.int32), kp, scale, (ch, cw), int(flip), geo
        masks = np.stack([np.asarray(m, np.uint8) for m in in_data[3]]) if len(in_data[3]) else np.zeros((0, H, W), np.uint8)
        out = img_u8, None, np.asarray(in_data[2], np.int32), masks, scale, (ch, cw), int(flip), geo
        if aug.copy_paste is not None:
            out += (decide_copy_paste(*aug.copy_paste, n_inst=masks.shape[0]),)
        return out

    def __call__(self, in_data, aug=None):
        if aug is not None and aug.lsj is not None:
            return self._lsj(in_data, aug)
        img = in_data[0]
        _, H, W = img.shape
        flip = bool(aug is not None and aug.flip)
        o_H, o_W = self.out_size(H, W, aug.min_size if aug is not None else None)
        scale = o_H / H
        img_u8 = np.ascontiguousarray(img.transpose(1, 2, 0)).astype(np.uint8)      # decoded JPEGs are integer-valued
        bbox = resize_bbox(flip_bbox(in_data[1], W) if flip else in_data[1], (H, W), (o_H, o_W))
        tail = () if aug is None else (int(flip),)
        if self.keypoints:
            keypoints = flip_keypoints(in_data[2], W, aug.keypoint_perm) if flip else in_data[2]
            keypoints = keypoints.astype(np.float32)
            kp = np.concatenate([keypoints[:, :, [1, 0]] * scale, keypoints[:, :, 2, None]], axis=2)
            return (img_u8, bbox, np.zeros(bbox.shape[0], dtype=np.int32), kp, scale, (o_H, o_W)) + tail
        bbox[:, 2:] = np.maximum(bbox[:, 2:], bbox[:, 2:] + 1)
        masks = np.stack([np.asarray(m, np.uint8) for m in in_data[3]]) if len(in_data[3]) else np.zeros((0, H, W), np.uint8)
        return (img_u8, bbox, np.asarray(in_data[2], np.int32), masks, scale, (o_H, o_W)) + tail
