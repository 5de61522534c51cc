"""PASCAL VOC instance-segmentation metric: the ChainerCV functions the reference's evaluator relies on (reference evaluator.py:5,
``chainercv.evaluations.eval_instance_segmentation_voc``, ``calc_instance_segmentation_voc_prec_rec``, ``calc_detection_voc_ap``,
``chainercv.utils.mask_iou``), with their signatures and matching rule.

The pixel work - intersections and areas between every predicted and every ground-truth mask at image resolution - runs on the
device (``_hip.ops.mask_iou_counts``, csrc/evaluate.hip); the IoU ``I / (Aa + Ab - I)`` is formed on the host in float64 from
those exact integer counts.  Matching and AP are host NumPy, as in ChainerCV:

* per image and class l, the predictions of class l are taken in descending score; each is matched to the ground truth of class
  l of largest IoU, or to none if that IoU is below ``iou_thresh``;
* a ground truth already taken makes a false positive (0); a difficult ground truth gives -1 (neither);
* a class with no non-difficult ground truth has no recall, so its AP is ``nan`` and ``map`` (``nanmean``) leaves it out.

Tie order: predictions of equal score keep their input order (a stable descending sort), both within an image and over the
whole split.  ChainerCV's ``argsort()[::-1]`` leaves the order of ties to NumPy's sort; results differ from it only on ties.
"""
from collections import defaultdict

import numpy as np


def _descending(score):
    """Indices of score in descending order; equal scores keep their input order."""
    return np.argsort(-np.asarray(score, dtype=np.float64), kind='stable')


def iou_from_counts(inter, area_a, area_b):
    """(Na, Nb) float64 IoU from integer counts: I / (Aa + Ab - I); 0 / 0 (two empty masks) is nan, as in ChainerCV."""
    inter = np.asarray(inter, dtype=np.float64)
    union = np.asarray(area_a, dtype=np.float64)[:, None] + np.asarray(area_b, dtype=np.float64)[None, :] - inter
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / union


def _device_masks(m, device=None):
    import torch
    if isinstance(m, torch.Tensor):
        return m if device is None else m.to(device)
    m = np.ascontiguousarray(m)
    if m.dtype != np.bool_:
        m = m != 0
    return torch.from_numpy(m).to(device if device is not None else torch.device('cuda', torch.cuda.current_device()))


def mask_iou(mask_a, mask_b):
    """IoU between every mask of mask_a (Na, H, W) and every mask of mask_b (Nb, H, W) -> (Na, Nb) float64.  Device tensors or
    NumPy arrays (copied to the current device); the counts are computed on the device."""
    from chainer_maskrcnn._hip import ops
    if tuple(mask_a.shape[1:]) != tuple(mask_b.shape[1:]):
        raise IndexError('mask_iou: masks of different sizes %s and %s' % (tuple(mask_a.shape), tuple(mask_b.shape)))
    a = _device_masks(mask_a)
    b = _device_masks(mask_b, a.device)
    inter, area_a, area_b = ops.mask_iou_counts(a, b)
    return iou_from_counts(inter.cpu().numpy(), area_a.cpu().numpy(), area_b.cpu().numpy())


class VOCMatchAccumulator(object):
    """Streaming state of the VOC metric: per class the number of non-difficult ground truths, and per prediction only its
    score and its match (1 true positive, 0 false positive, -1 difficult).  No mask is kept."""

    def __init__(self):
        self.n_pos = defaultdict(int)
        self.score = defaultdict(list)
        self.match = defaultdict(list)

    def add_image(self, iou, pred_label, pred_score, gt_label, gt_difficult=None, iou_thresh=0.5):
        """One image.  iou (D, G): IoU of prediction d and ground truth g (only entries of equal labels are read)."""
        pred_label = np.asarray(pred_label).reshape(-1)
        pred_score = np.asarray(pred_score).reshape(-1)
        gt_label = np.asarray(gt_label).reshape(-1)
        if gt_difficult is None:
            gt_difficult = np.zeros(gt_label.shape[0], dtype=bool)
        gt_difficult = np.asarray(gt_difficult, dtype=bool).reshape(-1)
        for l in np.unique(np.concatenate((pred_label, gt_label)).astype(int)):
            pk = np.flatnonzero(pred_label == l)
            pk = pk[_descending(pred_score[pk])]
            gk = np.flatnonzero(gt_label == l)
            gt_difficult_l = gt_difficult[gk]
            self.n_pos[l] += int(np.logical_not(gt_difficult_l).sum())
            self.score[l].extend(pred_score[pk].tolist())
            if len(pk) == 0:
                continue
            if len(gk) == 0:
                self.match[l].extend((0,) * len(pk))
                continue
            iou_l = np.asarray(iou)[np.ix_(pk, gk)]
            gt_index = iou_l.argmax(axis=1)
            gt_index[iou_l.max(axis=1) < iou_thresh] = -1
            selec = np.zeros(len(gk), dtype=bool)
            for gt_idx in gt_index:
                if gt_idx >= 0:
                    if gt_difficult_l[gt_idx]:
                        self.match[l].append(-1)
                    else:
                        self.match[l].append(0 if selec[gt_idx] else 1)
                    selec[gt_idx] = True
                else:
                    self.match[l].append(0)

    def prec_rec(self):
        """(prec, rec): lists indexed by class; None for a class never seen, rec None for a class without positives."""
        if not self.n_pos:
            return [], []
        n_fg_class = max(self.n_pos.keys()) + 1
        prec, rec = [None] * n_fg_class, [None] * n_fg_class
        for l in self.n_pos.keys():
            score_l = np.array(self.score[l], dtype=np.float64)
            match_l = np.array(self.match[l], dtype=np.int8)[_descending(score_l)]
            tp = np.cumsum(match_l == 1)
            fp = np.cumsum(match_l == 0)
            with np.errstate(divide='ignore', invalid='ignore'):
                prec[l] = tp / (fp + tp)            # a -1 prefix gives 0 / 0 = nan, as in ChainerCV
            if self.n_pos[l] > 0:
                rec[l] = tp / self.n_pos[l]
        return prec, rec


def calc_prec_rec_from_iou(ious, pred_labels, pred_scores, gt_labels, gt_difficults=None, iou_thresh=0.5):
    """calc_instance_segmentation_voc_prec_rec with the per-image IoU matrices (D_i, G_i) already computed (host only)."""
    acc = VOCMatchAccumulator()
    if gt_difficults is None:
        gt_difficults = [None] * len(gt_labels)
    for iou, pl, ps, gl, gd in zip(ious, pred_labels, pred_scores, gt_labels, gt_difficults):
        acc.add_image(iou, pl, ps, gl, gd, iou_thresh)
    return acc.prec_rec()


def _image_iou(pred_mask, pred_label, gt_mask, gt_label):
    """(D, G) IoU of one image on the device; pairs of different labels are skipped by the kernel (their entries are 0)."""
    import torch
    from chainer_maskrcnn._hip import ops
    D, G = len(pred_label), len(gt_label)
    if D == 0 or G == 0:
        return np.zeros((D, G), dtype=np.float64)
    a = _device_masks(pred_mask)
    b = _device_masks(gt_mask, a.device)
    lab = lambda x: torch.as_tensor(np.asarray(x, dtype=np.int32)).to(a.device) if not isinstance(x, torch.Tensor) else x.to(a.device)
    inter, area_a, area_b = ops.mask_iou_counts(a, b, lab(pred_label), lab(gt_label))
    return iou_from_counts(inter.cpu().numpy(), area_a.cpu().numpy(), area_b.cpu().numpy())


def _host(x):
    import torch
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def calc_instance_segmentation_voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults=None,
                                            iou_thresh=0.5):
    """Precision and recall per class over a dataset (ChainerCV's signature): iterables of per-image (D,H,W) masks, (D,) labels,
    (D,) scores, (G,H,W) masks, (G,) labels and optionally (G,) difficult flags.  Masks may be device tensors or NumPy arrays."""
    acc = VOCMatchAccumulator()
    if gt_difficults is None:
        gt_difficults = iter(lambda: None, 0)
    for pm, pl, ps, gm, gl, gd in zip(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults):
        iou = _image_iou(pm, pl, gm, gl)
        acc.add_image(iou, _host(pl), _host(ps), _host(gl), None if gd is None else _host(gd), iou_thresh)
    return acc.prec_rec()


def calc_detection_voc_ap(prec, rec, use_07_metric=False):
    """Average precision per class from prec / rec lists (ChainerCV's): area under the interpolated precision-recall curve, or the
    11-point VOC2007 metric.  nan for a class whose prec or rec is None."""
    n_fg_class = len(prec)
    ap = np.empty(n_fg_class)
    for l in range(n_fg_class):
        if prec[l] is None or rec[l] is None:
            ap[l] = np.nan
            continue
        if use_07_metric:
            ap[l] = 0
            for t in np.arange(0., 1.1, 0.1):
                if np.sum(rec[l] >= t) == 0:
                    p = 0
                else:
                    p = np.max(np.nan_to_num(prec[l])[rec[l] >= t])
                ap[l] += p / 11
        else:
            mpre = np.concatenate(([0], np.nan_to_num(prec[l]), [0]))
            mrec = np.concatenate(([0], rec[l], [1]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            i = np.where(mrec[1:] != mrec[:-1])[0]
            ap[l] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


def nanmean(ap):
    """map: mean AP over the classes that have one (nan for none at all, without a warning)."""
    ap = np.asarray(ap, dtype=np.float64)
    ok = ~np.isnan(ap)
    return float(ap[ok].mean()) if ok.any() else float('nan')


def eval_instance_segmentation_voc(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults=None, iou_thresh=0.5,
                                   use_07_metric=False):
    """{'ap': (n_fg_class,) ndarray, 'map': float} (ChainerCV's signature and result)."""
    prec, rec = calc_instance_segmentation_voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults,
                                                        iou_thresh=iou_thresh)
    ap = calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)
    return {'ap': ap, 'map': nanmean(ap)}
