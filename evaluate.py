#!/usr/bin/env python3
"""Scores a trained Mask R-CNN checkpoint with COCO's box and mask AP (pycocotools COCOeval, iouType 'segm' and 'bbox', over IoU
.50:.95) and writes its detections in COCO's results format, without pycocotools.  Flags in the style of train.py.

  python evaluate.py --weight result/model_90000.npz --synthetic 0 --anno-dir data/annotations --img-dir data --data-type 2017

--synthetic 0 evaluates every image of <anno-dir>/instances_<split><data-type>.json (COCOeval's default image set), the first
--eval-images of them when given; --synthetic 1 the deterministic make_batch val split of train.py --eval-metric mask_coco.  Writes
<out>/segm_results.json and <out>/bbox_results.json ({"image_id", "category_id", "segmentation": RLE / "bbox", "score"}; not with
--no-results) and <out>/metrics.json (all 12 stats per type, and the test-time augmentation under "tta" when it is on), and prints
COCOeval's summary lines.  --boundary 1 adds Boundary AP (Cheng et al., CVPR 2021): a third block of lines and a "boundary" entry in
metrics.json.  --tta-sizes / --tta-hflip 1 score with test-time augmentation (MaskRCNN.use_test_augmentation):

  python evaluate.py --weight result/model_90000.npz --tta-sizes 640 800 1000 --tta-hflip 1  Keypoint heads are scored by
train_keypoints.py --eval-metric keypoint_coco.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))
sys.path.insert(0, ROOT)

from chainer_maskrcnn.inference_options import (add_boundary_flag, add_boxpost_flags, add_dcn_flags, boundary_iou_types, add_extension_flags, add_tta_flags, boxpost_settings, build_inference_model, dcn_settings_of,  # noqa: E402
                                                extension_settings, read_labels, tta_settings, use_boxpost, use_tta)

SYNTHETIC_VAL_IMAGES = 16           # train.py's synthetic val split of --eval-images 0


def build_parser():
    parser = argparse.ArgumentParser(description='Mask R-CNN: COCO box and mask AP of a checkpoint')
    parser.add_argument('--gpu', '-g', type=int, default=0)
    parser.add_argument('--weight', '-w', type=str, default='', help='a Chainer-NPZ snapshot (train.py model_<iteration>.npz)')
    parser.add_argument('--label_file', '-f', type=str, default='data/label_coco.txt')
    parser.add_argument('--backbone', type=str, default='fpn')
    parser.add_argument('--head-arch', '-a', type=str, default='fpn')
    parser.add_argument('--synthetic', type=int, default=0, help='1: the synthetic val split; 0: COCO from --anno-dir / --img-dir')
    parser.add_argument('--anno-dir', default='data/annotations')
    parser.add_argument('--img-dir', default='data')
    parser.add_argument('--data-type', default='2017')
    parser.add_argument('--split', default='val', choices=['val', 'validation', 'train'])
    parser.add_argument('--eval-images', type=int, default=0, help='the first N images (0: all; --synthetic 1: %d)' % SYNTHETIC_VAL_IMAGES)
    parser.add_argument('--image-size', type=int, nargs=2, default=[800, 800], help='--synthetic 1: image height and width')
    parser.add_argument('--score-thresh', type=float, default=None, help="overrides the 'evaluate' preset's score threshold (0.05)")
    parser.add_argument('--no-results', action='store_true', help='do not write the COCO results files')
    add_extension_flags(parser)
    add_dcn_flags(parser)
    add_tta_flags(parser)
    add_boxpost_flags(parser)
    add_boundary_flag(parser)
    parser.add_argument('--out', '-o', default='result_eval', help='Output directory')
    return parser


def check_args(args):
    if args.head_arch == 'fpn_keypoint':
        raise ValueError('evaluate.py scores mask heads; keypoint heads are scored by train_keypoints.py --eval-metric keypoint_coco')
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world > 1:
        raise ValueError('evaluate.py runs in a single process; with %d ranks it is not supported' % world)
    extension_settings(args)
    dcn_settings_of(args)
    boundary_iou_types(args.boundary)
    return boxpost_settings(args.soft_nms, args.soft_nms_sigma, args.box_vote_thresh, args.max_detections)


def build_model(args):
    """MaskRCNN of the flags, with --weight loaded and the 'evaluate' preset (score threshold overridden by --score-thresh)."""
    return build_inference_model(args, 'evaluate')


def build_dataset(args, n_fg_class):
    from chainer_maskrcnn.evaluator import SyntheticCOCOEvalDataset
    if args.synthetic:
        H, W = args.image_size
        return SyntheticCOCOEvalDataset(args.eval_images or SYNTHETIC_VAL_IMAGES, H, W, n_fg_class=n_fg_class)
    from chainer_maskrcnn.dataset.coco_dataset import COCOInstanceEvalDataset
    return COCOInstanceEvalDataset(anno_dir=args.anno_dir, img_dir=args.img_dir, split=args.split, data_type=args.data_type,
                                   category_filter=read_labels(args.label_file), n=args.eval_images or None)


def run(args):
    """Evaluates and writes the files; returns {'segm': 12 stats, 'bbox': 12 stats} (and 'boundary' with --boundary 1)."""
    from chainer_maskrcnn import evaluations
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, split_coco_results
    boxpost = check_args(args)
    model = build_model(args)
    use_boxpost(model, boxpost)
    tta = tta_settings(args.tta_sizes, args.tta_hflip, args.tta_max_size, model.min_size)
    use_tta(model, tta)
    data = build_dataset(args, model.n_class - 1)
    results = None if args.no_results else []
    iou_types = boundary_iou_types(args.boundary)
    ev = InstanceSegmentationCOCOEvaluator(data, model, results=results, iou_types=iou_types)
    ev.evaluate()
    os.makedirs(args.out, exist_ok=True)
    if results is not None:
        segm, bbox = split_coco_results(results)
        for name, res in (('segm_results.json', segm), ('bbox_results.json', bbox)):
            with open(os.path.join(args.out, name), 'w') as f:
                json.dump(res, f)
    with open(os.path.join(args.out, 'metrics.json'), 'w') as f:
        extra = {k: v for k, v in (('tta', tta), ('boxpost', boxpost)) if v is not None}
        json.dump(dict(ev.stats, **extra) if extra else ev.stats, f, indent=1)
    for t in iou_types:
        print(evaluations.format_coco_stats(ev.stats[t], t))
    return ev.stats


def main():
    run(build_parser().parse_args())


if __name__ == '__main__':
    main()
