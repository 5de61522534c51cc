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
"""
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


class InstanceSegmentationVOCEvaluator(object):
    """PASCAL VOC mAP of ``target.predict`` over ``dataset``, whose examples are (img (3,H,W) 0..255, gt_masks (G,H,W), gt_labels (G,))
    or the same with (G,) difficult flags appended.  ``evaluate()`` returns {'main/map': float, 'main/ap/<label_names[l]>': float};
    a trainer writes them with the prefix 'validation/' (the reference's keys, e.g. 'validation/main/map').

    ``target``'s preset (score / NMS thresholds) is used as it is, and its training state is restored afterwards."""

    default_name = 'validation'

    def __init__(self, dataset, target, iou_thresh=0.5, use_07_metric=False, label_names=None):
        self.dataset = dataset
        self.target = target
        self.iou_thresh = iou_thresh
        self.use_07_metric = use_07_metric
        self.label_names = label_names

    def evaluate(self):
        from chainer_maskrcnn.nn import core
        target = self.target
        rpn, head = getattr(target, 'rpn', None), getattr(target, 'head', None)
        keep = (target.train, core.TRAIN, getattr(rpn, 'train', None), getattr(head, 'train', None))
        acc = evaluations.VOCMatchAccumulator()
        try:
            with torch.no_grad():
                for i in range(len(self.dataset)):
                    self._add_example(acc, self.dataset[i])
        finally:
            target.train, core.TRAIN = keep[0], keep[1]
            if keep[2] is not None:
                rpn.train = keep[2]
            if keep[3] is not None:
                head.train = keep[3]
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
        img = torch.as_tensor(np.asarray(img, dtype=np.float32)) if not isinstance(img, torch.Tensor) else img.to(torch.float32)
        masks, labels, scores = self.target.predict([img])
        mask, label, score = masks[0], labels[0].to(torch.int32), scores[0].to(torch.float32)
        gt_label = np.asarray(gt_label.cpu() if isinstance(gt_label, torch.Tensor) else gt_label, dtype=np.int32).reshape(-1)
        D, G = int(label.shape[0]), int(gt_label.shape[0])
        parts = [label, score.view(torch.int32)]
        if D and G:
            gm = gt_mask.to(dev) if isinstance(gt_mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(gt_mask)).to(dev)
            inter, area_a, area_b = ops.mask_iou_counts(mask, gm, label, torch.from_numpy(gt_label).to(dev))
            parts += [inter.reshape(-1), area_a, area_b]
        host = torch.cat(parts).cpu().numpy() if D else np.zeros((0,), dtype=np.int32)      # the one copy of this image
        pred_label, pred_score = host[:D], host[D:2 * D].view(np.float32)
        if D and G:
            o = 2 * D
            iou = evaluations.iou_from_counts(host[o:o + D * G].reshape(D, G), host[o + D * G:o + D * G + D], host[o + D * G + D:])
        else:
            iou = np.zeros((D, G), dtype=np.float64)
        acc.add_image(iou, pred_label, pred_score, gt_label, gt_difficult, self.iou_thresh)


class SyntheticEvalDataset(object):
    """Deterministic synthetic val split (utils/synthetic.make_batch, one image per seed): examples (img 0..255, masks, labels).
    Seeds start at ``first_seed``, far from the seeds of train.py's synthetic training pool."""

    def __init__(self, n_images, H, W, n_fg_class=80, G=8, first_seed=1000003):
        self.n, self.H, self.W, self.n_fg_class, self.G, self.first_seed = n_images, H, W, n_fg_class, G, first_seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from chainer_maskrcnn.utils.synthetic import make_batch
        if not 0 <= i < self.n:
            raise IndexError(i)
        b = make_batch(self.first_seed + i, 1, self.H, self.W, G=self.G, n_fg_class=self.n_fg_class)
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


class KeypointCOCOEvaluator(object):
    """COCO keypoint AP (pycocotools COCOeval, iouType='keypoints'; evaluations.COCOKeypointMatchAccumulator) of
    ``target.predict_keypoints`` over ``dataset``, whose examples are (img (3,H,W) 0..255, gt_kp (G,K,3) (y,x,v), gt_area (G,),
    gt_crowd (G,), gt_bbox_xywh (G,4)).  ``evaluate()`` returns {'main/map' (AP at OKS .50:.95), 'main/ap50', 'main/ap75',
    'main/ap_medium', 'main/ap_large', 'main/ar'}; a trainer writes them with the prefix 'validation/'.

    Per image: ``predict_keypoints``, then ONE device->host copy of the scores and the (y, x) of the (up to) 20 best-scored
    detections; OKS in float64 and the matching on the host.  sigmas default to COCO's 17; other K need explicit sigmas.
    ``target``'s preset is used as it is, and its training state is restored afterwards."""

    default_name = 'validation'

    def __init__(self, dataset, target, sigmas=None):
        K = getattr(getattr(target, 'head', None), 'n_keypoints', None)
        if sigmas is None and K is not None and K != len(evaluations.COCO_KEYPOINT_SIGMAS):
            raise ValueError('KeypointCOCOEvaluator: COCO defines OKS sigmas for its %d keypoints only; this model has %d - pass sigmas'
                             % (len(evaluations.COCO_KEYPOINT_SIGMAS), K))
        self.dataset = dataset
        self.target = target
        self.sigmas = None if sigmas is None else np.asarray(sigmas, dtype=np.float64)

    def evaluate(self):
        from chainer_maskrcnn.nn import core
        target = self.target
        rpn, head = getattr(target, 'rpn', None), getattr(target, 'head', None)
        keep = (target.train, core.TRAIN, getattr(rpn, 'train', None), getattr(head, 'train', None))
        acc = evaluations.COCOKeypointMatchAccumulator()
        try:
            with torch.no_grad():
                for i in range(len(self.dataset)):
                    self._add_example(acc, self.dataset[i])
        finally:
            target.train, core.TRAIN = keep[0], keep[1]
            if keep[2] is not None:
                rpn.train = keep[2]
            if keep[3] is not None:
                head.train = keep[3]
        s = acc.summarize()
        return {'main/map': s['AP'], 'main/ap50': s['AP50'], 'main/ap75': s['AP75'], 'main/ap_medium': s['APm'],
                'main/ap_large': s['APl'], 'main/ar': s['AR']}

    def _add_example(self, acc, example):
        img, gt_kp, gt_area, gt_crowd, gt_bbox = example[:5]
        img = torch.as_tensor(np.asarray(img, dtype=np.float32)) if not isinstance(img, torch.Tensor) else img.to(torch.float32)
        keypoints, _, scores = self.target.predict_keypoints([img])
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


class SyntheticKeypointEvalDataset(object):
    """Deterministic synthetic keypoint val split (utils/synthetic.make_batch with n_fg_class=1, n_keypoints=K, one image per seed):
    examples (img 0..255, gt_kp (G,K,3) (y,x,v=2), gt_area, gt_crowd (zeros), gt_bbox_xywh).  gt_area is the box area h * w, a
    stand-in for COCO's segmentation area.  Seeds start at ``first_seed``, far from the seeds of train.py's synthetic training pool."""

    def __init__(self, n_images, H, W, n_keypoints=17, G=8, first_seed=1000003):
        self.n, self.H, self.W, self.K, self.G, self.first_seed = n_images, H, W, n_keypoints, G, first_seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from chainer_maskrcnn.utils.synthetic import make_batch
        if not 0 <= i < self.n:
            raise IndexError(i)
        b = make_batch(self.first_seed + i, 1, self.H, self.W, G=self.G, n_fg_class=1, n_keypoints=self.K)
        box = b['bboxes'][0].astype(np.float64)
        h, w = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        xywh = np.stack([box[:, 1], box[:, 0], w, h], axis=1)
        return b['imgs'][0] * 255, b['keypoints'][0].astype(np.float64), h * w, np.zeros(self.G, dtype=bool), xywh
