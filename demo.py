#!/usr/bin/env python3
"""Draws what a Mask R-CNN / Keypoint R-CNN checkpoint detects in images: masks, contours, boxes and labels (or keypoint skeletons)
composed on the device by csrc/vis.hip (chainer_maskrcnn/vis.py), one PNG per image.  Flags in the style of evaluate.py.

  python demo.py --weight result/model_90000.npz photo1.jpg photos/ --out result_demo
  python demo.py --weight result/model_90000.npz --synthetic 4 --image-size 480 640 --json 1
  python demo.py --weight result_kp/model_90000.npz --head-arch fpn_keypoint photos/ --kp-thresh 2

inputs are image files and / or directories (their image files, sorted); --synthetic N draws on N images of the synthetic generator
instead.  Per image: predict (predict_keypoints for --head-arch fpn_keypoint) with the 'visualize' preset (score threshold 0.7 unless
--score-thresh), the picture drawn on the device, one device->host copy of the finished (H,W,3) picture, <out>/<stem>.png.  --json 1 also
writes <out>/<stem>.json: per detection the box as [x, y, w, h], category id and name, score, and for mask models the COCO run-length
code (the device encoder of the results export) or for keypoint models the keypoints.  --tta-sizes / --tta-hflip 1 predict with
test-time augmentation as evaluate.py does.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chainer_maskrcnn.inference_options import (add_boxpost_flags, add_dcn_flags, add_extension_flags, add_tta_flags, boxpost_settings, build_inference_model, dcn_settings_of,  # noqa: E402
                                                extension_settings, read_labels, tta_settings, use_boxpost, use_score_preset, use_tta)

IMAGE_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')
SYNTHETIC_FIRST_SEED = 2000003      # far from the seeds of the synthetic training pool and of the synthetic val split
VISUALIZE_SCORE_THRESH = 0.7        # MaskRCNN.use_preset('visualize')
DEFAULT_KP_THRESH = 2.0             # a keypoint is drawn when its heat-map logit reaches this


def build_parser():
    parser = argparse.ArgumentParser(description='Mask R-CNN: pictures of a checkpoint\'s detections')
    parser.add_argument('inputs', nargs='*', help='image files and / or directories of image files')
    parser.add_argument('--synthetic', type=int, default=0, metavar='N', help='N images of the synthetic generator instead of files')
    parser.add_argument('--gpu', '-g', type=int, default=0)
    parser.add_argument('--weight', '-w', type=str, default='', help='a Chainer-NPZ snapshot (train.py model_<iteration>.npz)')
    parser.add_argument('--label_file', '-f', type=str, default='data/label_coco.txt')
    parser.add_argument('--backbone', type=str, default='fpn')
    parser.add_argument('--head-arch', '-a', type=str, default='fpn')
    parser.add_argument('--out', '-o', default='result_demo', help='Output directory')
    parser.add_argument('--score-thresh', type=float, default=None,
                        help="overrides the 'visualize' preset's score threshold (%s)" % VISUALIZE_SCORE_THRESH)
    parser.add_argument('--alpha', type=float, default=0.5, help='opacity of the masks (keypoint heads: of limbs and keypoints)')
    parser.add_argument('--color-by', default='class', choices=['class', 'instance'])
    parser.add_argument('--no-masks', action='store_true')
    parser.add_argument('--no-boxes', action='store_true')
    parser.add_argument('--no-labels', action='store_true')
    parser.add_argument('--no-contours', action='store_true')
    parser.add_argument('--kp-thresh', type=float, default=None,
                        help='keypoint heads: the heat-map logit from which a keypoint is drawn (%s)' % DEFAULT_KP_THRESH)
    add_extension_flags(parser)
    add_dcn_flags(parser)
    add_tta_flags(parser)
    add_boxpost_flags(parser)
    parser.add_argument('--json', type=int, default=0, choices=[0, 1], help='1: also write <stem>.json per image')
    parser.add_argument('--image-size', type=int, nargs=2, default=[480, 640], help='--synthetic: image height and width')
    return parser


def collect_inputs(inputs):
    """The image files named by the positional arguments, directories expanded (sorted).  ValueError for a path that does not exist,
    cannot be read, is no image file, or a directory without image files."""
    files = []
    for p in inputs:
        if os.path.isdir(p):
            found = sorted(os.path.join(p, f) for f in os.listdir(p) if f.lower().endswith(IMAGE_EXTENSIONS))
            if not found:
                raise ValueError('%s: a directory without image files (%s)' % (p, ' '.join(IMAGE_EXTENSIONS)))
            files += found
        elif os.path.isfile(p):
            files.append(p)
        else:
            raise ValueError('%s: no such file or directory' % p)
    from PIL import Image
    for f in files:
        try:
            with Image.open(f) as im:
                im.verify()
        except Exception as e:
            raise ValueError('%s: not a readable image (%s)' % (f, e))
    return files


def check_args(args):
    """Every flag error, as ValueError, before the model is built.  Returns the list of input files (empty for --synthetic)."""
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world > 1:
        raise ValueError('demo.py runs in a single process; with %d ranks it is not supported' % world)
    if args.synthetic < 0:
        raise ValueError('--synthetic must not be negative, got %d' % args.synthetic)
    if args.synthetic and args.inputs:
        raise ValueError('--synthetic draws on generated images; it does not go with input files')
    if not args.synthetic and not args.inputs:
        raise ValueError('nothing to draw on: give image files or directories, or --synthetic N')
    if any(s <= 0 for s in args.image_size):
        raise ValueError('--image-size: height and width must be positive, got %s' % (args.image_size,))
    if not 0.0 <= args.alpha <= 1.0:
        raise ValueError('--alpha must lie in [0, 1], got %s' % args.alpha)
    if args.score_thresh is not None and not 0.0 <= args.score_thresh <= 1.0:
        raise ValueError('--score-thresh must lie in [0, 1], got %s' % args.score_thresh)
    if args.head_arch == 'fpn_keypoint':
        for flag in ('no_masks', 'no_contours', 'no_labels'):
            if getattr(args, flag):
                raise ValueError('--%s: a keypoint head draws boxes, limbs and keypoints; it has no masks, contours or labels to '
                                 'leave out' % flag.replace('_', '-'))
        if args.color_by != 'class':
            raise ValueError('--color-by: a keypoint head colours limbs and keypoints by their index')
    elif args.kp_thresh is not None:
        raise ValueError('--kp-thresh needs a keypoint head (--head-arch fpn_keypoint)')
    if args.tta_sizes and any(s <= 0 for s in args.tta_sizes):
        raise ValueError('--tta-sizes: every size must be positive, got %s' % (args.tta_sizes,))
    tta_settings(args.tta_sizes, args.tta_hflip, args.tta_max_size, 1)      # a max size without views
    boxpost_settings(args.soft_nms, args.soft_nms_sigma, args.box_vote_thresh, args.max_detections)
    extension_settings(args)
    dcn_settings_of(args)
    return collect_inputs(args.inputs)


def build_model(args):
    """MaskRCNN of the flags with --weight loaded; a keypoint head is COCO's: one class, 17 keypoints.  run() sets the 'visualize' preset
    on what this returns.  Tests replace this function to draw with a reduced network."""
    return build_inference_model(args)


def images(args, files):
    """(stem, (3,H,W) float32 RGB 0..255) per image, read or generated one at a time."""
    if args.synthetic:
        from chainer_maskrcnn.utils.synthetic import make_batch
        H, W = args.image_size
        for i in range(args.synthetic):
            yield 'synthetic_%04d' % i, np.ascontiguousarray(make_batch(SYNTHETIC_FIRST_SEED + i, 1, H, W)['imgs'][0] * 255, np.float32)
        return
    from chainer_maskrcnn.dataset.coco_dataset import read_image
    seen = {}
    for f in files:
        stem = os.path.splitext(os.path.basename(f))[0]
        seen[stem] = seen.get(stem, 0) + 1
        yield (stem if seen[stem] == 1 else '%s_%d' % (stem, seen[stem])), read_image(f)


def _xywh(yx):
    return [[float(b[1]), float(b[0]), float(b[3] - b[1]), float(b[2] - b[0])] for b in yx]


def draw_image(model, img, args, names=None):
    """predict and draw one image: returns (picture (H,W,3) uint8 device tensor, the JSON record of the detections)."""
    from chainer_maskrcnn import vis
    from chainer_maskrcnn._hip import ops
    x = torch.from_numpy(img).to(model.device)
    H, W = int(x.shape[1]), int(x.shape[2])
    if model.head_arch == 'fpn_keypoint':
        kps, labels, scores = model.predict_keypoints([x])
        bbox = model.last_bboxes[0]
        kp = kps[0].cpu().numpy()
        pic = vis.draw_keypoints(x, kp, bbox, scores[0], kp_thresh=DEFAULT_KP_THRESH if args.kp_thresh is None else args.kp_thresh,
                                 alpha=args.alpha, draw_boxes=not args.no_boxes)
        extra = [{'keypoints': [[float(v) for v in row] for row in k]} for k in kp]
    else:
        masks, labels, scores = model.predict([x])
        bbox = model.last_bboxes[0]
        pic = vis.draw_instances(x, masks[0], bbox, labels[0], scores[0], label_names=names, alpha=args.alpha, color_by=args.color_by,
                                 draw_masks=not args.no_masks, draw_boxes=not args.no_boxes, draw_labels=not args.no_labels,
                                 draw_contours=not args.no_contours)
        extra = []
        if args.json and int(labels[0].shape[0]):
            from chainer_maskrcnn.dataset.coco_api import rle_to_strings
            D = int(labels[0].shape[0])
            offsets, counts, area = ops.mask_rle_encode(masks[0])
            rle = torch.cat((offsets, counts, area)).cpu().numpy()
            strings = rle_to_strings(rle[:D + 1], rle[D + 1:len(rle) - D])
            extra = [{'segmentation': {'size': [H, W], 'counts': s.decode('ascii') if isinstance(s, bytes) else s}, 'area': int(a)}
                     for s, a in zip(strings, rle[len(rle) - D:])]
    record = None
    if args.json:
        lab, sc = labels[0].cpu().numpy(), scores[0].cpu().numpy()
        dets = []
        for d, box in enumerate(_xywh(bbox.cpu().numpy())):
            l = int(lab[d])
            det = {'bbox': box, 'category_id': l, 'category_name': names[l] if names and l < len(names) else str(l), 'score': float(sc[d])}
            if extra:
                det.update(extra[d])
            dets.append(det)
        record = {'height': H, 'width': W, 'detections': dets}
    return pic, record


def run(args):
    """Draws every image and writes the files; returns the list of files written."""
    from PIL import Image
    files = check_args(args)
    model = build_model(args)
    use_score_preset(model, 'visualize', args.score_thresh)
    use_boxpost(model, boxpost_settings(args.soft_nms, args.soft_nms_sigma, args.box_vote_thresh, args.max_detections))
    use_tta(model, tta_settings(args.tta_sizes, args.tta_hflip, args.tta_max_size, model.min_size))
    names = ['person'] if model.head_arch == 'fpn_keypoint' else read_labels(args.label_file)
    os.makedirs(args.out, exist_ok=True)
    written = []
    with torch.no_grad():
        for stem, img in images(args, files):
            pic, record = draw_image(model, img, args, names)
            path = os.path.join(args.out, stem + '.png')
            Image.fromarray(pic.cpu().numpy()).save(path)                  # the one device->host copy of the picture
            written.append(path)
            if record is not None:
                path = os.path.join(args.out, stem + '.json')
                with open(path, 'w') as f:
                    json.dump(record, f)
                written.append(path)
    return written


def main():
    for path in run(build_parser().parse_args()):
        print(path)


if __name__ == '__main__':
    main()
