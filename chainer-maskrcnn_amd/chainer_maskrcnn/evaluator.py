"""Validation metrics during training.  Mask heads: the reference's ``InstanceSegmentationVOCEvaluator`` (reference evaluator.py, a copy of
ChainerCV's; attached to the val split in reference train.py:113-115,164-166), streaming.

The reference runs ``apply_to_iterator(target.predict, ...)`` and keeps every predicted mask of the split in host memory before
``eval_instance_segmentation_voc``.  Here each image is predicted, matched and dropped: the predicted masks stay on the device, the
mask-IoU counts are computed there (``mask_iou_counts``, labels on, so cross-class pairs cost nothing), and the only copy to the
host per image beyond ``predict``'s own is one buffer holding the (D, G) intersections, the areas, the labels and the scores.
What is kept is one (score, match) per prediction and the positive count per class (evaluations.VOCMatchAccumulator).

Keypoint heads: ``KeypointCOCOEvaluator``, COCO's keypoint AP (pycocotools COCOeval, iouType='keypoints') of
``predict_keypoints``; the heat maps are decoded on the device (``keypoint_decode``) and one copy per image brings the scores and
keypoint positions of the 20 best detections to the host, where OKS and the matching run in float64.

Mask heads, COCO's metric: ``InstanceSegmentationCOCOEvaluator``, mask and box AP over IoU .50:.95 (pycocotools COCOeval, iouType
'segm' / 'bbox'), from the same device counts; optionally it writes COCO results entries, the masks run-length encoded on the device
(``mask_rle_encode``).
"""
import contextlib

import numpy as np
import torch

from chainer_maskrcnn import evaluations
from chainer_maskrcnn._hip import ops


def coco_mask_example(example):
    """A COCOMaskLoader example (img, bbox, label, [masks]) -> the evaluator's (img, gt_masks (G, H, W), gt_labels), like the
    reference's EvaluatorTransform (train.py:40-47); an image without instances gets a (0, H, W) mask array."""
    img, _, label, masks = example
    img = np.asarray(img)
    gt = np.stack(masks) if len(masks) else np.zeros((0,) + img.shape[1:], dtype=np.uint8)
    return img, gt, np.asarray(label, dtype=np.int32)


class TransformedDataset(object):
    """dataset[i] -> transform(dataset[i]) for the first n examples (all when n is None)."""

    def __init__(self, dataset, transform, n=None):
        self.dataset, self.transform = dataset, transform
        self.n = len(dataset) if n is None else min(n, len(dataset))

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return self.transform(self.dataset[i])


def image_tensor(img):
    """An example's image (array or tensor, 0..255) as the float32 tensor ``predict`` / ``predict_keypoints`` take."""
    return img.to(torch.float32) if isinstance(img, torch.Tensor) else torch.as_tensor(np.asarray(img, dtype=np.float32))


def device_tensor(a, device):
    """Ground truth (array or tensor) on the device."""
    return a.to(device) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def copy_to_host(*parts):
    """int32 / float32 device tensors -> NumPy arrays of their shapes and dtypes through ONE device->host copy (none when every part is
    empty): concatenated as 32-bit words on the device, split by lengths on the host."""
    if any(p.dtype not in (torch.int32, torch.float32) for p in parts):
        raise TypeError('copy_to_host: int32 / float32 tensors expected, got %s' % ', '.join(str(p.dtype) for p in parts))
    dtypes = [np.float32 if p.dtype == torch.float32 else np.int32 for p in parts]
    if not any(p.numel() for p in parts):
        return [np.zeros(tuple(p.shape), dtype=t) for p, t in zip(parts, dtypes)]
    words = torch.cat([p.reshape(-1).view(torch.int32) for p in parts]).cpu().numpy()
    words = np.split(words, np.cumsum([p.numel() for p in parts])[:-1])
    return [w.view(t).reshape(tuple(p.shape)) for w, p, t in zip(words, parts, dtypes)]


@contextlib.contextmanager
def training_state_kept(target):
    """``target.train``, ``core.TRAIN`` and the train flags a forward leaves on ``target.rpn`` / ``target.head`` (where the target has
    them) are, after the block, what they were before it - also when the block raises."""
    from chainer_maskrcnn.nn import core
    parts = [p for p in (getattr(target, 'rpn', None), getattr(target, 'head', None)) if hasattr(p, 'train')]
    keep = (target.train, core.TRAIN, [p.train for p in parts])
    try:
        yield
    finally:
        target.train, core.TRAIN = keep[0], keep[1]
        for p, t in zip(parts, keep[2]):
            p.train = t


class _Evaluator(object):
    """The loop of the three evaluators: every example of ``dataset`` through ``_add_example`` into a fresh ``_accumulator()``, without
    autograd and with the target's training state restored afterwards, then ``_report`` of what was accumulated."""

    default_name = 'validation'

    def evaluate(self):
        acc = self._accumulator()
        with training_state_kept(self.target), torch.no_grad():
            for i in range(len(self.dataset)):
                self._add_example(acc, self.dataset[i])
        return self._report(acc)


class _SyntheticSplit(object):
    """A deterministic synthetic val split: example i is ``_example`` of utils/synthetic.make_batch(first_seed + i, 1, H, W, G=G,
    **batch_kwargs), one image per seed.  Seeds start at ``first_seed``, far from the seeds of train.py's synthetic training pool."""

    def __init__(self, n_images, H, W, G, first_seed, **batch_kwargs):
        self.n, self.H, self.W, self.G, self.first_seed, self.batch_kwargs = n_images, H, W, G, first_seed, batch_kwargs

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from chainer_maskrcnn.utils.synthetic import make_batch
        if not 0 <= i < self.n:
            raise IndexError(i)
        return self._example(make_batch(self.first_seed + i, 1, self.H, self.W, G=self.G, **self.batch_kwargs), i)


class InstanceSegmentationVOCEvaluator(_Evaluator):
    """PASCAL VOC mAP of ``target.predict`` over ``dataset``, whose examples are (img (3,H,W) 0..255, gt_masks (G,H,W), gt_labels (G,))
    or the same with (G,) difficult flags appended.  ``evaluate()`` returns {'main/map': float, 'main/ap/<label_names[l]>': float};
    a trainer writes them with the prefix 'validation/' (the reference's keys, e.g. 'validation/main/map').

    ``target``'s preset (score / NMS thresholds) is used as it is, and its training state is restored afterwards."""

    def __init__(self, dataset, target, iou_thresh=0.5, use_07_metric=False, label_names=None):
        self.dataset = dataset
        self.target = target
        self.iou_thresh = iou_thresh
        self.use_07_metric = use_07_metric
        self.label_names = label_names

    def _accumulator(self):
        return evaluations.VOCMatchAccumulator()

    def _report(self, acc):
        prec, rec = acc.prec_rec()
        ap = evaluations.calc_detection_voc_ap(prec, rec, use_07_metric=self.use_07_metric)
        report = {'main/map': evaluations.nanmean(ap)}
        if self.label_names is not None:
            for l, name in enumerate(self.label_names):
                report['main/ap/%s' % name] = float(ap[l]) if l < len(ap) else float('nan')
        return report

    def _add_example(self, acc, example):
        img, gt_mask, gt_label = example[:3]
        gt_difficult = np.asarray(example[3], dtype=bool) if len(example) > 3 and example[3] is not None else None
        dev = self.target.device
        masks, labels, scores = self.target.predict([image_tensor(img)])
        mask, label, score = masks[0], labels[0].to(torch.int32), scores[0].to(torch.float32)
        gt_label = np.asarray(gt_label.cpu() if isinstance(gt_label, torch.Tensor) else gt_label, dtype=np.int32).reshape(-1)
        D, G = int(label.shape[0]), int(gt_label.shape[0])
        if D and G:
            overlap = ops.mask_iou_counts(mask, device_tensor(gt_mask, dev), label, torch.from_numpy(gt_label).to(dev))
            pred_label, pred_score, inter, area_a, area_b = copy_to_host(label, score, *overlap)      # the one copy of this image
            iou = evaluations.iou_from_counts(inter, area_a, area_b)
        else:
            pred_label, pred_score = copy_to_host(label, score)
            iou = np.zeros((D, G), dtype=np.float64)
        acc.add_image(iou, pred_label, pred_score, gt_label, gt_difficult, self.iou_thresh)


class SyntheticEvalDataset(_SyntheticSplit):
    """Deterministic synthetic val split (_SyntheticSplit): examples (img 0..255, masks, labels)."""

    def __init__(self, n_images, H, W, n_fg_class=80, G=8, first_seed=1000003):
        super().__init__(n_images, H, W, G, first_seed, n_fg_class=n_fg_class)
        self.n_fg_class = n_fg_class

    def _example(self, b, i):
        return b['imgs'][0] * 255, b['masks'][0], b['labels'][0]


# ---- COCO keypoint AP ----------------------------------------------------------------------------------------------------------------
def coco_keypoint_example(loader, i):
    """Example i of a COCOKeypointsLoader as the keypoint evaluator's (img, gt_kp (G, K, 3) (y, x, v), gt_area (G,), gt_crowd (G,),
    gt_bbox_xywh (G, 4)): COCO's (x, y, v) keypoints in (y, x, v) order, the annotations' own area, iscrowd and raw bbox."""
    img, _, kp = loader.get_example(i)
    ann = loader.get_annotations(i)
    kp = np.asarray(kp, dtype=np.float64).reshape(-1, loader.n_keypoints, 3)
    return img, kp[:, :, [1, 0, 2]], ann['area'], ann['iscrowd'], ann['bbox']


class COCOKeypointEvalDataset(object):
    """The first n examples (all when n is None) of a COCOKeypointsLoader through coco_keypoint_example."""

    def __init__(self, loader, n=None):
        self.loader = loader
        self.n = len(loader) if n is None else min(n, len(loader))

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return coco_keypoint_example(self.loader, i)


class KeypointCOCOEvaluator(_Evaluator):
    """COCO keypoint AP (pycocotools COCOeval, iouType='keypoints'; evaluations.COCOKeypointMatchAccumulator) of
    ``target.predict_keypoints`` over ``dataset``, whose examples are (img (3,H,W) 0..255, gt_kp (G,K,3) (y,x,v), gt_area (G,),
    gt_crowd (G,), gt_bbox_xywh (G,4)).  ``evaluate()`` returns {'main/map' (AP at OKS .50:.95), 'main/ap50', 'main/ap75',
    'main/ap_medium', 'main/ap_large', 'main/ar'}; a trainer writes them with the prefix 'validation/'.

    Per image: ``predict_keypoints``, then ONE device->host copy of the scores and the (y, x) of the (up to) 20 best-scored
    detections; OKS in float64 and the matching on the host.  sigmas default to COCO's 17; other K need explicit sigmas.
    ``target``'s preset is used as it is, and its training state is restored afterwards."""

    def __init__(self, dataset, target, sigmas=None):
        K = getattr(getattr(target, 'head', None), 'n_keypoints', None)
        if sigmas is None and K is not None and K != len(evaluations.COCO_KEYPOINT_SIGMAS):
            raise ValueError('KeypointCOCOEvaluator: COCO defines OKS sigmas for its %d keypoints only; this model has %d - pass sigmas'
                             % (len(evaluations.COCO_KEYPOINT_SIGMAS), K))
        self.dataset = dataset
        self.target = target
        self.sigmas = None if sigmas is None else np.asarray(sigmas, dtype=np.float64)

    def _accumulator(self):
        return evaluations.COCOKeypointMatchAccumulator()

    def _report(self, acc):
        s = acc.summarize()
        return {'main/map': s['AP'], 'main/ap50': s['AP50'], 'main/ap75': s['AP75'], 'main/ap_medium': s['APm'],
                'main/ap_large': s['APl'], 'main/ar': s['AR']}

    def _add_example(self, acc, example):
        img, gt_kp, gt_area, gt_crowd, gt_bbox = example[:5]
        keypoints, _, scores = self.target.predict_keypoints([image_tensor(img)])
        kp, score = keypoints[0], scores[0].to(torch.float32)
        D, K = int(kp.shape[0]), int(kp.shape[1])
        n = min(D, acc.max_dets)
        if D:
            top = torch.sort(score, descending=True, stable=True)[1][:n]        # equal scores keep their order (COCOeval's mergesort)
            host = torch.cat((score[top], kp[top][:, :, :2].reshape(-1))).cpu().numpy()      # the one copy of this image
        else:
            host = np.zeros((0,), dtype=np.float32)
        dt_score, dt_yx = host[:n], host[n:].reshape(n, K, 2)
        evaluations.add_keypoint_image(acc, dt_yx, dt_score, gt_kp, gt_area, gt_crowd, gt_bbox, self.sigmas)


class SyntheticKeypointEvalDataset(_SyntheticSplit):
    """Deterministic synthetic keypoint val split (_SyntheticSplit with n_fg_class=1, n_keypoints=K): examples (img 0..255, gt_kp (G,K,3)
    (y,x,v=2), gt_area, gt_crowd (zeros), gt_bbox_xywh).  gt_area is the box area h * w, a stand-in for COCO's segmentation area."""

    def __init__(self, n_images, H, W, n_keypoints=17, G=8, first_seed=1000003):
        super().__init__(n_images, H, W, G, first_seed, n_fg_class=1, n_keypoints=n_keypoints)
        self.K = n_keypoints

    def _example(self, b, i):
        box = b['bboxes'][0].astype(np.float64)
        h, w = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        xywh = np.stack([box[:, 1], box[:, 0], w, h], axis=1)
        return b['imgs'][0] * 255, b['keypoints'][0].astype(np.float64), h * w, np.zeros(self.G, dtype=bool), xywh


# ---- COCO box and mask AP ------------------------------------------------------------------------------------------------------------
_COCO_KEYS = (('map', 'AP'), ('ap50', 'AP50'), ('ap75', 'AP75'), ('ap_small', 'APs'), ('ap_medium', 'APm'), ('ap_large', 'APl'),
              ('ar', 'AR100'))


class InstanceSegmentationCOCOEvaluator(_Evaluator):
    """COCO mask and box AP (pycocotools COCOeval, iouType 'segm' / 'bbox'; evaluations.COCOInstanceMatchAccumulator) of
    ``target.predict`` over ``dataset``, whose examples are (img (3,H,W) 0..255, gt_masks (G,H,W), gt_labels (G,), gt_area (G,),
    gt_crowd (G,), gt_bbox_xywh (G,4), image_id) - COCOInstanceEvalDataset, SyntheticCOCOEvalDataset.  ``cat_ids[label]`` is a
    label's COCO category id (default: ``dataset.cat_ids``, else the label itself).

    ``evaluate()`` returns, for 'segm', {'main/map' (AP at IoU .50:.95), 'main/ap50', 'main/ap75', 'main/ap_small', 'main/ap_medium',
    'main/ap_large', 'main/ar' (AR at 100 detections)}, the same keys under 'main/bbox/' for 'bbox', and 'main/ap/<label_names[l]>'
    (segm AP of category l) when label_names is given; ``self.stats`` keeps all 12 stats of each type.  A trainer writes them with the
    prefix 'validation/'.

    Per image: ``predict``, then ``mask_iou_counts`` with labels on (exact intersections and areas on the device), then ONE copy to the
    host of the labels, scores, boxes, intersections and areas; IoU in float64 and the matching on the host.  With ``results`` a list,
    also ``mask_rle_encode`` on the device and one more copy (offsets and counts); one COCO results entry per detection is appended:
    {'image_id', 'category_id', 'segmentation': {'size': [H, W], 'counts': <compressed RLE>}, 'bbox': [x, y, w, h], 'score'}
    (split_coco_results makes the two results files).  No mask is kept on the host.  ``target``'s preset is used as it is, and its
    training state is restored afterwards.

    With 'boundary' among ``iou_types`` (off by default) Boundary AP (Cheng et al., CVPR 2021) is reported under
    'main/boundary/': segm's matching on min(mask IoU, boundary-band IoU).  The per-image device call is then
    ``mask_boundary_iou_counts``, whose three band arrays ride in the same copy; the 'segm' and 'bbox' numbers do not change."""

    def __init__(self, dataset, target, label_names=None, cat_ids=None, iou_types=('segm', 'bbox'), results=None):
        if not iou_types or any(t not in ('segm', 'bbox', 'boundary') for t in iou_types):
            raise ValueError("InstanceSegmentationCOCOEvaluator: iou_types from ('segm', 'bbox', 'boundary'), got %r" % (iou_types,))
        self.dataset = dataset
        self.target = target
        self.label_names = label_names
        self.cat_ids = list(cat_ids) if cat_ids is not None else getattr(dataset, 'cat_ids', None)
        self.iou_types = tuple(iou_types)
        self.results = results
        self.stats = {}

    def _cat(self, label):
        label = np.asarray(label, dtype=np.int64)
        return label if self.cat_ids is None else np.asarray(self.cat_ids, dtype=np.int64)[label]

    def _accumulator(self):
        return {t: evaluations.COCOInstanceMatchAccumulator() for t in self.iou_types}

    def _report(self, accs):
        report = {}
        for t, acc in accs.items():
            pr = acc.precision_recall()
            s = self.stats[t] = acc.summarize(pr)
            prefix = 'main/' if t == 'segm' else 'main/%s/' % t
            report.update({prefix + k: s[name] for k, name in _COCO_KEYS})
            if t == 'segm' and self.label_names is not None:
                ap = acc.category_ap(pr)
                for l, name in enumerate(self.label_names):
                    report['main/ap/%s' % name] = ap.get(int(self._cat(l)), -1.0)
        return report

    def _add_example(self, accs, example):
        img, gt_mask, gt_label, gt_area, gt_crowd, gt_bbox, image_id = example[:7]
        dev = self.target.device
        masks, labels, scores = self.target.predict([image_tensor(img)])
        mask, label, score = masks[0], labels[0].to(torch.int32).contiguous(), scores[0].to(torch.float32).contiguous()
        gt_label = np.asarray(gt_label.cpu() if isinstance(gt_label, torch.Tensor) else gt_label, dtype=np.int32).reshape(-1)
        gt_crowd = np.asarray(gt_crowd, dtype=bool).reshape(-1)
        gt_area = np.asarray(gt_area, dtype=np.float64).reshape(-1)
        D, G = int(label.shape[0]), int(gt_label.shape[0])
        H, W = int(mask.shape[1]), int(mask.shape[2])
        if D:
            bbox = self.target.last_bboxes[0].to(torch.float32).contiguous()
            counts = ops.mask_boundary_iou_counts if 'boundary' in accs else ops.mask_iou_counts
            overlap = counts(mask, device_tensor(gt_mask, dev).reshape(G, H, W), label, torch.from_numpy(gt_label).to(dev))
            dt_label, dt_score, yx, inter_h, area_dt_h, area_gt_h, *band_h = copy_to_host(label, score, bbox, *overlap)     # the one copy of this image
            yx = yx.astype(np.float64)
            xywh = np.stack([yx[:, 1], yx[:, 0], yx[:, 3] - yx[:, 1], yx[:, 2] - yx[:, 0]], axis=1)
        else:
            dt_label, dt_score = np.zeros((0,), np.int32), np.zeros((0,), np.float32)
            xywh, inter_h, area_dt_h, area_gt_h = np.zeros((0, 4)), np.zeros((0, G)), np.zeros((0,)), np.zeros((G,))
            band_h = [inter_h, area_dt_h, area_gt_h]
        dt_cat, gt_cat = self._cat(dt_label), self._cat(gt_label)
        for t, acc in accs.items():
            if t == 'segm':
                iou, dt_area = evaluations.segm_iou_from_counts(inter_h, area_dt_h, area_gt_h, gt_crowd), area_dt_h
            elif t == 'boundary':
                iou, dt_area = evaluations.boundary_iou_from_counts(inter_h, area_dt_h, area_gt_h, *band_h, gt_crowd), area_dt_h
            else:
                iou, dt_area = evaluations.bbox_iou_xywh(xywh, gt_bbox, gt_crowd), xywh[:, 2] * xywh[:, 3]
            acc.add_image(iou, dt_cat, dt_score, dt_area, gt_cat, gt_area, gt_crowd)
        if self.results is not None and D:
            from chainer_maskrcnn.dataset.coco_api import rle_to_strings
            offsets, counts, _ = ops.mask_rle_encode(mask)
            strings = rle_to_strings(*copy_to_host(offsets, counts))           # the second copy: the run lengths
            for d in range(D):
                self.results.append({'image_id': int(image_id), 'category_id': int(dt_cat[d]),
                                     'segmentation': {'size': [H, W], 'counts': strings[d]},
                                     'bbox': [float(v) for v in xywh[d]], 'score': float(dt_score[d])})


def split_coco_results(results):
    """The evaluator's results list as the two COCO results lists (segm: without boxes, so that COCO.loadRes ranges a detection by
    its pixel count; bbox: without masks)."""
    segm = [{k: r[k] for k in ('image_id', 'category_id', 'segmentation', 'score')} for r in results]
    bbox = [{k: r[k] for k in ('image_id', 'category_id', 'bbox', 'score')} for r in results]
    return segm, bbox


class SyntheticCOCOEvalDataset(_SyntheticSplit):
    """SyntheticEvalDataset with COCO's annotation fields: examples (img 0..255, masks, labels, area = each mask's pixel count, iscrowd
    (none), bbox_xywh from make_batch's boxes, image_id = the seed index).  Category ids are the labels."""

    def __init__(self, n_images, H, W, n_fg_class=80, G=8, first_seed=1000003):
        super().__init__(n_images, H, W, G, first_seed, n_fg_class=n_fg_class)
        self.n_fg_class = n_fg_class
        self.cat_ids = list(range(n_fg_class))

    def _example(self, b, i):
        masks, box = b['masks'][0], b['bboxes'][0].astype(np.float64)
        xywh = np.stack([box[:, 1], box[:, 0], box[:, 3] - box[:, 1], box[:, 2] - box[:, 0]], axis=1)
        area = (masks != 0).reshape(len(masks), -1).sum(axis=1).astype(np.float64)
        return b['imgs'][0] * 255, masks, b['labels'][0], area, np.zeros(len(masks), dtype=bool), xywh, i
