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


# ---- COCO keypoint AP (pycocotools COCOeval, iouType='keypoints') ----------------------------------------------------------------
# computeOks / evaluateImg / accumulate / summarize of pycocotools/cocoeval.py for ONE category (person), with its keypoint
# parameters: maxDets 20, OKS thresholds .50:.05:.95, 101 recall points, area ranges all / medium / large (closed intervals: a
# value is out of range when a < lo or a > hi).  Ground truth is ranged by its annotation area, a detection by the area of its
# keypoint extent box (loadRes).  Equal scores keep their input order within an image and image order across images (COCOeval's
# two mergesorts).

COCO_KEYPOINT_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
OKS_THRESHOLDS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
RECALL_THRESHOLDS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
KEYPOINT_AREA_RANGES = (('all', (0 ** 2, 1e5 ** 2)), ('medium', (32 ** 2, 96 ** 2)), ('large', (96 ** 2, 1e5 ** 2)))
KEYPOINT_MAX_DETS = 20


def keypoint_oks(dt_yx, gt_kp_yxv, gt_area, gt_bbox_xywh, sigmas=None):
    """(D, G) float64 object keypoint similarity (computeOks): dt_yx (D, K, 2) detected (y, x), gt_kp_yxv (G, K, 3) (y, x, v),
    gt_area (G,), gt_bbox_xywh (G, 4).  e = (dx^2 + dy^2) / (2 sigma)^2 / (area + eps) / 2; with labelled keypoints (v > 0) only
    those count, without any the distance is to the ground-truth box expanded to [x - w, x + 2w] x [y - h, y + 2h]; oks =
    mean(exp(-e)).  sigmas default to COCO's 17."""
    sigmas = COCO_KEYPOINT_SIGMAS if sigmas is None else np.asarray(sigmas, dtype=np.float64)
    dt = np.asarray(dt_yx, dtype=np.float64).reshape(-1, len(sigmas), 2)
    gt = np.asarray(gt_kp_yxv, dtype=np.float64).reshape(-1, len(sigmas), 3)
    gt_area = np.asarray(gt_area, dtype=np.float64).reshape(-1)
    gt_bbox = np.asarray(gt_bbox_xywh, dtype=np.float64).reshape(-1, 4)
    var = (sigmas * 2) ** 2
    yd, xd = dt[:, :, 0], dt[:, :, 1]
    oks = np.zeros((dt.shape[0], gt.shape[0]), dtype=np.float64)
    for j in range(gt.shape[0]):
        yg, xg, vg = gt[j, :, 0], gt[j, :, 1], gt[j, :, 2]
        vis = vg > 0
        if vis.any():
            dx, dy = xd - xg, yd - yg
        else:
            bx, by, bw, bh = gt_bbox[j]
            x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
            dx = np.maximum(0, x0 - xd) + np.maximum(0, xd - x1)
            dy = np.maximum(0, y0 - yd) + np.maximum(0, yd - y1)
        e = (dx ** 2 + dy ** 2) / var / (gt_area[j] + np.spacing(1)) / 2
        if vis.any():
            e = e[:, vis]
        oks[:, j] = np.exp(-e).sum(axis=1) / e.shape[1]
    return oks


def keypoint_extent_area(dt_yx):
    """(D,) area of each detection's keypoint extent box, (max x - min x) * (max y - min y): COCO.loadRes for keypoint results."""
    dt = np.asarray(dt_yx, dtype=np.float64)
    if dt.shape[0] == 0:
        return np.zeros((0,), dtype=np.float64)
    return (dt[:, :, 1].max(1) - dt[:, :, 1].min(1)) * (dt[:, :, 0].max(1) - dt[:, :, 0].min(1))


class COCOKeypointMatchAccumulator(object):
    """Streaming state of COCO keypoint AP (evaluateImg per image, accumulate at the end) for one category.  Kept per detection: its
    score and, per OKS threshold and area range, whether it matched a ground truth and whether it is ignored; per area range the
    number of ground truths that are not ignored.  No keypoints or heat maps are kept."""

    def __init__(self, max_dets=KEYPOINT_MAX_DETS, oks_thresholds=OKS_THRESHOLDS, area_ranges=KEYPOINT_AREA_RANGES):
        self.max_dets = max_dets
        self.thresholds = np.asarray(oks_thresholds, dtype=np.float64)
        self.area_ranges = [tuple(r) for _, r in area_ranges]
        self.area_names = [n for n, _ in area_ranges]
        A = len(self.area_ranges)
        self.scores = []                                  # per image, (D_i,) in evaluateImg's order
        self.matched = [[] for _ in range(A)]             # per area range, per image (T, D_i) bool
        self.ignored = [[] for _ in range(A)]
        self.n_pos = np.zeros(A, dtype=np.int64)          # per area range: ground truths not ignored
        self.n_images = 0                                 # images with a detection or a ground truth (COCOeval's non-None evalImgs)

    def add_image(self, oks, dt_score, dt_area, gt_area, gt_ignore, gt_crowd):
        """One image.  oks (D, G): OKS of detection d (input order) and ground truth g; dt_score (D,), dt_area (D,) (keypoint extent
        areas); gt_area (G,); gt_ignore (G,) crowd or no labelled keypoint; gt_crowd (G,) (a crowd may absorb several detections)."""
        dt_score = np.asarray(dt_score, dtype=np.float64).reshape(-1)
        dt_area = np.asarray(dt_area, dtype=np.float64).reshape(-1)
        gt_area = np.asarray(gt_area, dtype=np.float64).reshape(-1)
        gt_ignore = np.asarray(gt_ignore, dtype=bool).reshape(-1)
        gt_crowd = np.asarray(gt_crowd, dtype=bool).reshape(-1)
        D, G, T = dt_score.shape[0], gt_area.shape[0], len(self.thresholds)
        if D == 0 and G == 0:
            return
        self.n_images += 1
        order = np.argsort(-dt_score, kind='mergesort')[:self.max_dets]
        score, dt_area = dt_score[order], dt_area[order]
        oks = np.asarray(oks, dtype=np.float64).reshape(D, G)[order] if D and G else np.zeros((len(order), G))
        self.scores.append(score)
        for a, (lo, hi) in enumerate(self.area_ranges):
            g_ig = gt_ignore | (gt_area < lo) | (gt_area > hi)
            gorder = np.argsort(g_ig, kind='mergesort')           # not ignored first
            g_ig, crowd = g_ig[gorder], gt_crowd[gorder]
            o = oks[:, gorder]
            self.n_pos[a] += int(np.count_nonzero(~g_ig))
            nd = len(order)
            dtm = np.zeros((T, nd), dtype=bool)
            dt_ig = np.zeros((T, nd), dtype=bool)
            if nd and G:
                for t, thr in enumerate(self.thresholds):
                    gtm = np.zeros(G, dtype=bool)
                    for d in range(nd):
                        best, m = min(thr, 1 - 1e-10), -1
                        for g in range(G):
                            if gtm[g] and not crowd[g]:
                                continue                          # taken, and not a crowd
                            if m > -1 and not g_ig[m] and g_ig[g]:
                                break                             # a real match found; only ignored ones remain
                            if o[d, g] < best:
                                continue
                            best, m = o[d, g], g
                        if m == -1:
                            continue
                        dt_ig[t, d] = g_ig[m]
                        dtm[t, d] = True
                        gtm[m] = True
            out = (dt_area < lo) | (dt_area > hi)
            dt_ig |= ~dtm & out[None, :]
            self.matched[a].append(dtm)
            self.ignored[a].append(dt_ig)

    def precision_recall(self):
        """COCOeval.accumulate: precision (T, R, A) at the 101 recall points and recall (T, A); -1 where an area range has no ground
        truth that counts (or no image was added)."""
        T, R, A = len(self.thresholds), len(RECALL_THRESHOLDS), len(self.area_ranges)
        precision = -np.ones((T, R, A))
        recall = -np.ones((T, A))
        if self.n_images == 0:
            return precision, recall
        scores = np.concatenate(self.scores) if self.scores else np.zeros((0,))
        inds = np.argsort(-scores, kind='mergesort')
        for a in range(A):
            npig = int(self.n_pos[a])
            if npig == 0:
                continue
            dtm = np.concatenate(self.matched[a], axis=1)[:, inds]
            dt_ig = np.concatenate(self.ignored[a], axis=1)[:, inds]
            tps = np.logical_and(dtm, np.logical_not(dt_ig))
            fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
            tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
            fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
            for t in range(T):
                tp, fp = tp_sum[t], fp_sum[t]
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, a] = rc[-1] if nd else 0
                pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr        # precision envelope (right to left)
                ri = np.searchsorted(rc, RECALL_THRESHOLDS, side='left')
                q = np.zeros(R)
                ok = ri < nd
                q[ok] = pr[ri[ok]]
                precision[t, :, a] = q
        return precision, recall

    def summarize(self):
        """COCOeval.summarize for keypoints: {'AP', 'AP50', 'AP75', 'APm', 'APl', 'AR', 'AR50', 'AR75', 'ARm', 'ARl'}; a mean over
        the cells that are not -1, -1 when there is none."""
        precision, recall = self.precision_recall()
        t50, t75 = int(np.argmin(np.abs(self.thresholds - .5))), int(np.argmin(np.abs(self.thresholds - .75)))
        a_all, a_m, a_l = (self.area_names.index(n) for n in ('all', 'medium', 'large'))

        def mean(s):
            s = s[s > -1]
            return float(np.mean(s)) if s.size else -1.0
        return {'AP': mean(precision[:, :, a_all]), 'AP50': mean(precision[t50, :, a_all]), 'AP75': mean(precision[t75, :, a_all]),
                'APm': mean(precision[:, :, a_m]), 'APl': mean(precision[:, :, a_l]),
                'AR': mean(recall[:, a_all]), 'AR50': mean(recall[t50, a_all]), 'AR75': mean(recall[t75, a_all]),
                'ARm': mean(recall[:, a_m]), 'ARl': mean(recall[:, a_l])}


def eval_keypoint_coco(dt_yx, dt_scores, gt_kp_yxv, gt_areas, gt_crowds, gt_bboxes_xywh, sigmas=None):
    """COCO keypoint AP over a dataset (iterables of per-image (D, K, 2) detected (y, x), (D,) scores, (G, K, 3) ground-truth
    (y, x, v), (G,) areas, (G,) crowd flags, (G, 4) boxes (x, y, w, h)).  Ground truth without a labelled keypoint is ignored, as
    COCO's num_keypoints == 0.  Returns COCOKeypointMatchAccumulator.summarize()'s dict."""
    acc = COCOKeypointMatchAccumulator()
    for dt, sc, gt, ga, gc, gb in zip(dt_yx, dt_scores, gt_kp_yxv, gt_areas, gt_crowds, gt_bboxes_xywh):
        add_keypoint_image(acc, dt, sc, gt, ga, gc, gb, sigmas)
    return acc.summarize()


def add_keypoint_image(acc, dt_yx, dt_score, gt_kp_yxv, gt_area, gt_crowd, gt_bbox_xywh, sigmas=None):
    """One image into a COCOKeypointMatchAccumulator: OKS of the (up to max_dets) best-scored detections, then the matching."""
    K = len(COCO_KEYPOINT_SIGMAS if sigmas is None else sigmas)
    dt_yx = np.asarray(dt_yx, dtype=np.float64).reshape(-1, K, 2)
    dt_score = np.asarray(dt_score, dtype=np.float64).reshape(-1)
    gt = np.asarray(gt_kp_yxv, dtype=np.float64).reshape(-1, K, 3)
    gt_crowd = np.asarray(gt_crowd, dtype=bool).reshape(-1)
    gt_ignore = gt_crowd | ((gt[:, :, 2] > 0).sum(1) == 0)
    top = np.argsort(-dt_score, kind='mergesort')[:acc.max_dets]           # computeOks's cut; add_image sorts again (stable)
    dt_yx, dt_score = dt_yx[top], dt_score[top]
    oks = keypoint_oks(dt_yx, gt, gt_area, gt_bbox_xywh, sigmas) if len(top) and len(gt) else np.zeros((len(top), len(gt)))
    acc.add_image(oks, dt_score, keypoint_extent_area(dt_yx), gt_area, gt_ignore, gt_crowd)


# ---- COCO box and mask AP (pycocotools COCOeval, iouType='segm' / 'bbox', useCats=1) -------------------------------------------------
# evaluateImg / accumulate / summarize of pycocotools/cocoeval.py with its default parameters: IoU thresholds .50:.05:.95, 101 recall
# points, maxDets (1, 10, 100), area ranges all / small / medium / large (closed intervals), per (image, category) the detections in
# descending score (a stable sort: equal scores keep their input order) cut at 100, ground truth ignored when it is a crowd (which can
# absorb several detections) and sorted after the rest.  IoU is maskApi.c's: I / (A_dt + A_gt - I), or I / A_dt for a crowd, and 0
# when the masks (boxes) do not overlap.  Ground truth is ranged by its annotation area, a segm detection by its pixel count, a bbox
# detection by w * h (COCO.loadRes).

COCO_IOU_THRESHOLDS = OKS_THRESHOLDS
COCO_AREA_RANGES = (('all', (0 ** 2, 1e5 ** 2)), ('small', (0 ** 2, 32 ** 2)), ('medium', (32 ** 2, 96 ** 2)), ('large', (96 ** 2, 1e5 ** 2)))
COCO_MAX_DETS = (1, 10, 100)
COCO_STAT_NAMES = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')


def segm_iou_from_counts(inter, dt_area, gt_area, gt_crowd):
    """(D, G) float64 mask IoU from exact integer counts (maskApi.c rleIou): I / (A_dt + A_gt - I), I / A_dt for crowd ground truth,
    0 where I == 0 (empty masks included)."""
    inter = np.asarray(inter, dtype=np.float64).reshape(len(dt_area), len(gt_area))
    da = np.asarray(dt_area, dtype=np.float64).reshape(-1, 1)
    ga = np.asarray(gt_area, dtype=np.float64).reshape(1, -1)
    union = np.where(np.asarray(gt_crowd, dtype=bool).reshape(1, -1), da, da + ga - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(inter > 0, inter / union, 0.0)


# ---- Boundary IoU (Cheng et al., "Boundary IoU: Improving Object-Centric Image Segmentation Evaluation", CVPR 2021) ---------------------
# COCO's matching with another IoU: min(mask IoU, IoU of the two masks' boundary bands).  The band of a mask is what d erosions by a 3 x 3
# block of ones remove, the outside of the image counting as background; d = 2 % of the image diagonal.
BOUNDARY_DILATION_RATIO = 0.02


def boundary_dilation(H, W, ratio=BOUNDARY_DILATION_RATIO):
    """The band width d of an H x W image: int(round(ratio * sqrt(H^2 + W^2))) in float64 with Python's round (half to even), at
    least 1."""
    return max(int(round(float(ratio) * float(np.sqrt(np.float64(int(H)) * int(H) + np.float64(int(W)) * int(W))))), 1)


def mask_boundary(mask, dilation):
    """The boundary band of mask(s) (..., H, W) (any nonzero value is a set pixel) as bool: M & ~E, E[y, x] = 1 iff M is 1 on the whole
    (2 d + 1)^2 square around (y, x) and that square lies inside the image.  Separable: per axis a cumulative sum counts the set pixels
    of each 2 d + 1 window (two passes in all, whatever d)."""
    d = int(dilation)
    if d < 1:
        raise ValueError('mask_boundary: dilation %r < 1' % (dilation,))
    m = np.asarray(mask) != 0
    if m.ndim < 2:
        raise ValueError('mask_boundary: (..., H, W) masks expected, got %s' % (m.shape,))
    e = m
    for axis in (m.ndim - 1, m.ndim - 2):
        n = e.shape[axis]
        pad = [(0, 0)] * m.ndim
        pad[axis] = (d + 1, d)                                                # zeros outside the image; one more in front for the difference
        c = np.cumsum(np.pad(e, pad).astype(np.int32), axis=axis, dtype=np.int32)
        hi = np.take(c, np.arange(2 * d + 1, 2 * d + 1 + n), axis=axis)       # sum of positions <= i + d
        lo = np.take(c, np.arange(0, n), axis=axis)                           # sum of positions <  i - d
        e = (hi - lo) == 2 * d + 1
    return m & ~e


def boundary_iou_from_counts(inter, dt_area, gt_area, binter, dt_barea, gt_barea, gt_crowd):
    """(D, G) float64 Boundary IoU from exact integer counts: min(mask IoU, band IoU), each by segm_iou_from_counts' rule (I / (A_dt +
    A_gt - I), I / A_dt for crowd ground truth, 0 where I == 0) - the mask counts first, the band counts second."""
    return np.minimum(segm_iou_from_counts(inter, dt_area, gt_area, gt_crowd), segm_iou_from_counts(binter, dt_barea, gt_barea, gt_crowd))


def bbox_iou_xywh(dt_xywh, gt_xywh, gt_crowd):
    """(D, G) float64 box IoU of (x, y, w, h) boxes (maskApi.c bbIou): the overlap w * h over da + ga - overlap, or over da for crowd
    ground truth; 0 where the boxes do not overlap."""
    d = np.asarray(dt_xywh, dtype=np.float64).reshape(-1, 1, 4)
    g = np.asarray(gt_xywh, dtype=np.float64).reshape(1, -1, 4)
    w = np.minimum(d[..., 2] + d[..., 0], g[..., 2] + g[..., 0]) - np.maximum(d[..., 0], g[..., 0])
    h = np.minimum(d[..., 3] + d[..., 1], g[..., 3] + g[..., 1]) - np.maximum(d[..., 1], g[..., 1])
    i = w * h
    da, ga = d[..., 2] * d[..., 3], g[..., 2] * g[..., 3]
    u = np.where(np.asarray(gt_crowd, dtype=bool).reshape(1, -1), da, da + ga - i)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where((w > 0) & (h > 0), i / u, 0.0)


class COCOInstanceMatchAccumulator(object):
    """Streaming state of COCOeval for 'segm' or 'bbox' over all categories.  Per (image, category) with a detection, kept: the scores
    of its (up to 100) detections in evaluateImg's order and, per IoU threshold and area range, whether each matched and whether it is
    ignored; per (category, area range) the number of ground truths that are not ignored.  No mask or box is kept.

    The greedy matching of evaluateImg runs for all categories, thresholds and area ranges of an image at once: the image's
    detections are visited in descending score (which keeps each category's own order), and each takes, per (threshold, area range),
    the available same-category ground truth of largest IoU >= the threshold (the last one among equal IoUs), preferring ground truth
    that is not ignored - evaluateImg's loop over the ground truth sorted ignored-last."""

    def __init__(self, max_dets=COCO_MAX_DETS, iou_thresholds=COCO_IOU_THRESHOLDS, area_ranges=COCO_AREA_RANGES):
        self.max_dets = tuple(max_dets)
        self.thresholds = np.asarray(iou_thresholds, dtype=np.float64)
        self.area_names = [n for n, _ in area_ranges]
        self.lo = np.array([r[0] for _, r in area_ranges], dtype=np.float64)
        self.hi = np.array([r[1] for _, r in area_ranges], dtype=np.float64)
        self.entries = defaultdict(list)           # category -> per image with a detection: (scores (n,), matched (T,A,n), ignored (T,A,n))
        self.n_pos = defaultdict(lambda: np.zeros(len(self.lo), dtype=np.int64))      # category -> (A,) ground truths not ignored

    def add_image(self, iou, dt_cat, dt_score, dt_area, gt_cat, gt_area, gt_crowd):
        """One image.  iou (D, G): IoU of detection d (input order) and ground truth g (only same-category pairs are read); dt_cat (D,),
        dt_score (D,), dt_area (D,); gt_cat (G,), gt_area (G,) (annotation areas), gt_crowd (G,) (iscrowd: ignored, absorbs
        detections)."""
        dt_cat = np.asarray(dt_cat).reshape(-1).astype(np.int64)
        dt_score = np.asarray(dt_score, dtype=np.float64).reshape(-1)
        dt_area = np.asarray(dt_area, dtype=np.float64).reshape(-1)
        gt_cat = np.asarray(gt_cat).reshape(-1).astype(np.int64)
        gt_area = np.asarray(gt_area, dtype=np.float64).reshape(-1)
        gt_crowd = np.asarray(gt_crowd, dtype=bool).reshape(-1)
        D, G, T, A = dt_score.shape[0], gt_area.shape[0], len(self.thresholds), len(self.lo)
        g_ig = gt_crowd[None, :] | (gt_area[None, :] < self.lo[:, None]) | (gt_area[None, :] > self.hi[:, None])      # (A, G)
        for c in np.unique(gt_cat):
            self.n_pos[int(c)] += np.count_nonzero(~g_ig[:, gt_cat == c], axis=1)
        if D == 0:
            return
        order = np.argsort(-dt_score, kind='mergesort')
        cat_o = dt_cat[order]
        rank = np.zeros(D, dtype=np.int64)             # rank of each detection within its category, in score order
        for c in np.unique(cat_o):
            sel = cat_o == c
            rank[sel] = np.arange(np.count_nonzero(sel))
        keep = order[rank < self.max_dets[-1]]
        n = keep.shape[0]
        cat_k = dt_cat[keep]
        matched = np.zeros((T, A, n), dtype=bool)
        ignored = np.zeros((T, A, n), dtype=bool)
        if G:
            io = np.where(cat_k[:, None] == gt_cat[None, :], np.asarray(iou, dtype=np.float64).reshape(D, G)[keep], -1.0)
            thr = np.minimum(self.thresholds, 1 - 1e-10)[:, None, None]                # (T, 1, 1)
            taken = np.zeros((T, A, G), dtype=bool)
            rev = np.arange(G)[::-1]
            for j in np.flatnonzero((io >= thr.min()).any(axis=1)):
                ok = (io[j][None, None, :] >= thr) & (~taken | gt_crowd[None, None, :])          # (T, A, G)
                real = ok & ~g_ig[None]
                use = np.where(real.any(axis=-1, keepdims=True), real, ok & g_ig[None])
                val = np.where(use, io[j][None, None, :], -np.inf)[..., rev]
                m = G - 1 - np.argmax(val, axis=-1)                                     # the last maximum (T, A)
                found = use.any(axis=-1)
                ti, ai = np.nonzero(found)
                taken[ti, ai, m[ti, ai]] = True
                matched[:, :, j] = found
                ignored[:, :, j] = found & g_ig[np.arange(A)[None, :], m]
        out = (dt_area[keep][None, :] < self.lo[:, None]) | (dt_area[keep][None, :] > self.hi[:, None])     # (A, n)
        ignored |= ~matched & out[None]
        s = dt_score[keep]
        for c in np.unique(cat_k):
            sel = np.flatnonzero(cat_k == c)
            self.entries[int(c)].append((s[sel], matched[:, :, sel], ignored[:, :, sel]))

    def categories(self):
        """The categories seen (ground truth or detections), ascending: COCOeval's sorted catIds, less those never seen (whose cells
        are -1 and do not enter any mean)."""
        return sorted(set(self.n_pos) | set(self.entries))

    def precision_recall(self):
        """COCOeval.accumulate: precision (T, R, K, A, M) at the 101 recall points and recall (T, K, A, M), K = categories(), M =
        max_dets; -1 where a (category, area range) has no ground truth that counts."""
        cats = self.categories()
        T, R, K, A, M = len(self.thresholds), len(RECALL_THRESHOLDS), len(cats), len(self.lo), len(self.max_dets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        for k, c in enumerate(cats):
            npig = self.n_pos[c] if c in self.n_pos else np.zeros(A, dtype=np.int64)
            ents = self.entries.get(c, [])
            for mi, md in enumerate(self.max_dets):
                if ents:
                    scores = np.concatenate([e[0][:md] for e in ents])
                    inds = np.argsort(-scores, kind='mergesort')
                    dtm = np.concatenate([e[1][:, :, :md] for e in ents], axis=2)[:, :, inds]
                    dt_ig = np.concatenate([e[2][:, :, :md] for e in ents], axis=2)[:, :, inds]
                else:
                    dtm = dt_ig = np.zeros((T, A, 0), dtype=bool)
                tp_sum = np.cumsum(dtm & ~dt_ig, axis=2).astype(np.float64)
                fp_sum = np.cumsum(~dtm & ~dt_ig, axis=2).astype(np.float64)
                nd = tp_sum.shape[2]
                for a in range(A):
                    if npig[a] == 0:
                        continue
                    rc = tp_sum[:, a] / npig[a]                                          # (T, nd)
                    pr = tp_sum[:, a] / (fp_sum[:, a] + tp_sum[:, a] + np.spacing(1))
                    recall[:, k, a, mi] = rc[:, -1] if nd else 0
                    if nd:
                        pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]         # precision envelope (right to left)
                    for t in range(T):
                        ri = np.searchsorted(rc[t], RECALL_THRESHOLDS, side='left')
                        q = np.zeros(R)
                        ok = ri < nd
                        q[ok] = pr[t, ri[ok]]
                        precision[t, :, k, a, mi] = q
        return precision, recall

    def summarize(self, precision_recall=None):
        """COCOeval.summarize: {'AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl'}, each a mean
        over the cells that are not -1, -1.0 when there is none."""
        precision, recall = self.precision_recall() if precision_recall is None else precision_recall

        def stat(ap, thr=None, area='all', max_det=100):
            a, m = [self.area_names.index(area)], [self.max_dets.index(max_det)]
            s = precision if ap else recall
            if thr is not None:
                s = s[np.where(np.isclose(self.thresholds, thr))[0]]
            s = s[:, :, :, a, m] if ap else s[:, :, a, m]
            return float(np.mean(s[s > -1])) if s[s > -1].size else -1.0
        md = self.max_dets[-1]
        vals = (stat(1), stat(1, .5), stat(1, .75), stat(1, area='small'), stat(1, area='medium'), stat(1, area='large'),
                stat(0, max_det=self.max_dets[0]), stat(0, max_det=self.max_dets[1]), stat(0, max_det=md), stat(0, area='small'),
                stat(0, area='medium'), stat(0, area='large'))
        return dict(zip(COCO_STAT_NAMES, vals))

    def category_ap(self, precision_recall=None):
        """{category: AP over IoU .50:.95, area all, 100 detections} (-1.0 for a category without ground truth that counts)."""
        precision, _ = self.precision_recall() if precision_recall is None else precision_recall
        a, m = self.area_names.index('all'), len(self.max_dets) - 1
        out = {}
        for k, c in enumerate(self.categories()):
            s = precision[:, :, k, a, m]
            out[c] = float(np.mean(s[s > -1])) if s[s > -1].size else -1.0
        return out


def format_coco_stats(stats, iou_type):
    """COCOeval.summarize's twelve printed lines under an 'iouType: <iou_type>' line."""
    rows = (('Average Precision', '0.50:0.95', 'all', 100), ('Average Precision', '0.50', 'all', 100),
            ('Average Precision', '0.75', 'all', 100), ('Average Precision', '0.50:0.95', 'small', 100),
            ('Average Precision', '0.50:0.95', 'medium', 100), ('Average Precision', '0.50:0.95', 'large', 100),
            ('Average Recall', '0.50:0.95', 'all', 1), ('Average Recall', '0.50:0.95', 'all', 10), ('Average Recall', '0.50:0.95', 'all', 100),
            ('Average Recall', '0.50:0.95', 'small', 100), ('Average Recall', '0.50:0.95', 'medium', 100),
            ('Average Recall', '0.50:0.95', 'large', 100))
    lines = ['iouType: %s' % iou_type]
    for (title, iou, area, md), name in zip(rows, COCO_STAT_NAMES):
        lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
            title, '(AP)' if 'Precision' in title else '(AR)', iou, area, md, stats[name]))
    return '\n'.join(lines)


def _load_results(results):
    import json
    if isinstance(results, str):
        with open(results) as f:
            results = json.load(f)
    return list(results)


def evaluate_coco_results(gt_annotation_file, results, iou_type, img_ids=None):
    """COCOeval(cocoGt, cocoGt.loadRes(results), iou_type) over ``img_ids`` (default: every image of the annotation file) and all its
    categories, on the host ('boundary': a segm results file scored with min(mask IoU, band IoU), mask_boundary on the host): ``results`` is a COCO results file or list ({'image_id', 'category_id', 'segmentation' (RLE) or 'bbox',
    'score'}); masks are decoded with dataset.coco_api.  As in COCO.loadRes, a segm detection's area is its pixel count unless the
    results carry boxes too (then w * h: loadRes takes such a list as box results).  Returns summarize()'s dict of the 12 stats."""
    from chainer_maskrcnn.dataset.coco_api import COCO, rle_decode, rle_from_string
    if iou_type not in ('segm', 'bbox', 'boundary'):
        raise ValueError("evaluate_coco_results: iou_type 'segm', 'bbox' or 'boundary', got %r" % (iou_type,))
    gt = COCO(gt_annotation_file)
    cat_ids = set(gt.getCatIds())
    img_ids = sorted(set(gt.getImgIds() if img_ids is None else img_ids))
    res = _load_results(results)
    box_area = bool(res) and bool(res[0].get('bbox'))          # loadRes takes a list whose first entry has a box as box results
    by_img = defaultdict(list)
    for r in res:
        if r['category_id'] in cat_ids:
            by_img[r['image_id']].append(r)
    acc = COCOInstanceMatchAccumulator()
    for img_id in img_ids:
        info = gt.imgs[img_id]
        h, w = info['height'], info['width']
        anns = [a for a in gt.imgToAnns.get(img_id, ()) if a['category_id'] in cat_ids]
        dts = by_img.get(img_id, [])
        gt_cat = np.array([a['category_id'] for a in anns], np.int64)
        gt_area = np.array([a.get('area', 0.0) for a in anns], np.float64)
        gt_crowd = np.array([bool(a.get('iscrowd', 0)) for a in anns], bool)
        dt_cat = np.array([d['category_id'] for d in dts], np.int64)
        dt_score = np.array([d['score'] for d in dts], np.float64)
        if iou_type in ('segm', 'boundary'):
            def mask(s):
                c = s['counts']
                return rle_decode(rle_from_string(c) if isinstance(c, (str, bytes)) else np.asarray(c, np.int64), *s['size'])
            dm = np.array([mask(d['segmentation']) for d in dts], np.float64).reshape(len(dts), h * w)
            gm = np.array([gt.annToMask(a) for a in anns], np.float64).reshape(len(anns), h * w)
            dt_area = dm.sum(axis=1)
            iou = segm_iou_from_counts(dm @ gm.T, dt_area, gm.sum(axis=1), gt_crowd)
            if iou_type == 'boundary':
                d = boundary_dilation(h, w)
                db = mask_boundary(dm.reshape(-1, h, w), d).reshape(len(dts), h * w).astype(np.float64)
                gb = mask_boundary(gm.reshape(-1, h, w), d).reshape(len(anns), h * w).astype(np.float64)
                iou = np.minimum(iou, segm_iou_from_counts(db @ gb.T, db.sum(axis=1), gb.sum(axis=1), gt_crowd))
            if box_area:
                db = np.array([d['bbox'] for d in dts], np.float64).reshape(-1, 4)
                dt_area = db[:, 2] * db[:, 3]
        else:
            db = np.array([d['bbox'] for d in dts], np.float64).reshape(-1, 4)
            dt_area = db[:, 2] * db[:, 3]
            iou = bbox_iou_xywh(db, np.array([a['bbox'] for a in anns], np.float64).reshape(-1, 4), gt_crowd)
        acc.add_image(iou, dt_cat, dt_score, dt_area, gt_cat, gt_area, gt_crowd)
    return acc.summarize()
