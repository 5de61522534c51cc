#!/usr/bin/env python3
"""Cost of test-time augmentation (MaskRCNN.use_test_augmentation, csrc/tta.hip) on full ResNet-50-FPN Mask R-CNN, 81 classes.

--mode time (default): milliseconds per image of plain predict, one-view TTA (the model's min_size), hflip (V = 2) and sizes 640 / 800 /
  1000 with hflip (V = 6, long side <= --max-size-v6), over --images images after --warmup, alternating 480 x 640 and 640 x 427
  sources, in --repeats alternating repeats (one pass over the cases per repeat); device syncs around every case.  The score threshold
  is calibrated (bisection on plain predict) to give about --detections detections per image and is reported with the counts.
--mode profile: every new kernel on synthetic inputs of --views 2 or 8 views (300 proposals each, D = 100 detections) for a
  `rocprofv3 --kernel-trace --stats` run: the union class NMS runs at R = 300 * V (600 / 2400).  Seeded full-size weights give the RPN
  only a handful of proposals per image, so the model's own unions are too small to measure the union NMS.

Weights: seeded (--seed) or a train.py snapshot (--weight).  Prints one JSON object per measurement; --out FILE also writes them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _model(args):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    m = MaskRCNN(n_fg_class=80, device='cuda:0', seed=args.seed)
    if args.weight:
        from chainer_maskrcnn.utils.chainer_npz import load_npz
        load_npz(args.weight, m, strict=False)
    m.use_preset('evaluate')
    return m


def _images(n):
    rs = np.random.RandomState(0)
    shapes = [(480, 640), (640, 427)]
    return [torch.from_numpy((rs.rand(3, *shapes[i % 2]) * 255).astype(np.float32)).cuda() for i in range(n)]


def _mean_detections(m, imgs):
    _, labels, _ = m.predict(imgs)
    return float(np.mean([int(l.shape[0]) for l in labels]))


def _calibrate(m, imgs, target):
    """Bisection on the score threshold (plain predict on imgs) for about `target` detections per image."""
    lo, hi = 0.0, 1.0
    for _ in range(14):
        m.score_thresh = 0.5 * (lo + hi)
        if _mean_detections(m, imgs) > target:
            lo = m.score_thresh
        else:
            hi = m.score_thresh
    m.score_thresh = hi
    return hi


def _run(m, imgs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for img in imgs:
        _, labels, _ = m.predict([img])
        n += int(labels[0].shape[0])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(imgs), n / len(imgs)


def bench_time(args, emit):
    m = _model(args)
    imgs = _images(args.images)
    thresh = args.score_thresh if args.score_thresh is not None else _calibrate(m, imgs[:4], args.detections)
    m.score_thresh = thresh
    cases = [('predict', None), ('tta_1view', dict(sizes=[m.min_size])), ('tta_hflip_V2', dict(sizes=[m.min_size], hflip=True)),
             ('tta_640_800_1000_hflip_V6', dict(sizes=[640, 800, 1000], hflip=True, max_size=args.max_size_v6))]
    for name, kw in cases:                          # warm-up: every view size's kernels and allocations
        m.use_test_augmentation(**kw) if kw else m.use_test_augmentation(None)
        _run(m, imgs[:args.warmup])
    for rep in range(args.repeats):
        for name, kw in cases:
            m.use_test_augmentation(**kw) if kw else m.use_test_augmentation(None)
            ms, det = _run(m, imgs)
            emit({'case': name, 'repeat': rep, 'ms_per_image': round(ms, 3), 'detections_per_image': round(det, 1),
                  'score_thresh': thresh, 'images': len(imgs), 'sources': '480x640 / 640x427',
                  'views': 1 if kw is None else len(kw['sizes']) * (2 if kw.get('hflip') else 1),
                  'max_size': m.max_size if not kw or not kw.get('max_size') else kw['max_size']})
    m.use_test_augmentation(None)


def bench_profile(args, emit):
    """Every new kernel on synthetic inputs shaped like a V-view union of 300 proposals each (81 classes, softmax of N(0, 3^2) scores,
    score threshold 0.05) and D = 100 detections, --iters calls each: the union class NMS runs at R = 300 * V."""
    from chainer_maskrcnn._hip import ops
    from chainer_maskrcnn.dataset import augment
    V, R1, D, n_class, ld, loc0 = args.views, 300, 100, 81, 96, 88
    rs = np.random.RandomState(0)
    rois, box = [], []
    for v in range(V):
        c = rs.uniform(50, 550, (R1, 2)); hw = np.exp(rs.uniform(np.log(20), np.log(300), (R1, 2)))
        rois.append(torch.from_numpy(np.concatenate([c - hw / 2, c + hw / 2], 1).astype(np.float32)).cuda())
        b = np.zeros((R1, ld), np.float32)
        b[:, :n_class] = rs.standard_normal((R1, n_class)) * 3
        b[:, loc0:loc0 + 4] = rs.standard_normal((R1, 4)) * 0.5
        box.append(torch.from_numpy(b).cuda())
    mirrors = [v % 2 == 1 for v in range(V)]
    img = torch.from_numpy((rs.rand(3, 480, 640) * 255).astype(np.float32)).cuda()
    logits = [torch.from_numpy(rs.standard_normal((D, 28, 28, 96)).astype(np.float32)).cuda() for _ in range(V)]
    heat = [torch.from_numpy(rs.standard_normal((D, 56, 56, 32)).astype(np.float32)).cuda() for _ in range(V)]
    label = torch.from_numpy(rs.randint(0, 79, D).astype(np.int32)).cuda()
    y0, x0 = rs.uniform(0, 400, D), rs.uniform(0, 500, D)
    bbox = torch.from_numpy(np.stack([y0, x0, y0 + rs.uniform(20, 300, D), x0 + rs.uniform(20, 300, D)], 1).astype(np.float32)).cuda()
    perm = augment.flip_permutation(augment.COCO_KEYPOINT_NAMES)
    kept = 0
    for _ in range(args.iters):
        ops.image_resize_mirror_f32(img, 800, 1066, 1, 255.0)
        cb, pb = ops.tta_detect_decode(rois, box, mirrors, [1.25] * V, n_class, loc0, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), (480, 640))
        _, cnt = ops.class_nms_ws(cb, pb, 1, n_class - 1, 0.05, 0.3)
        p = ops.tta_mask_merge(logits, mirrors, label)
        ops.mask_paste_prob(p, bbox, (480, 640))
        ops.tta_keypoint_merge(heat, mirrors, 17, perm)
    kept = int(cnt.sum())
    candidates = int((pb[:, 1:n_class - 1] > 0.05).sum())
    torch.cuda.synchronize()
    emit({'mode': 'profile', 'views': V, 'union_rows': int(cb.shape[0]), 'candidates_above_0.05': candidates, 'kept': kept, 'D': D,
          'iters': args.iters})


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--mode', default='time', choices=['time', 'profile'])
    p.add_argument('--images', type=int, default=50)
    p.add_argument('--warmup', type=int, default=4)
    p.add_argument('--repeats', type=int, default=2)
    p.add_argument('--detections', type=float, default=100.0, help='calibration target: detections per image')
    p.add_argument('--score-thresh', type=float, default=None, help='skip the calibration')
    p.add_argument('--max-size-v6', type=int, default=1333, help='long-side cap of the V = 6 case')
    p.add_argument('--views', type=int, default=2, choices=[2, 8], help='--mode profile')
    p.add_argument('--iters', type=int, default=10, help='--mode profile: calls of each kernel')
    p.add_argument('--seed', type=int, default=1234)
    p.add_argument('--weight', default='')
    p.add_argument('--out', default='')
    args = p.parse_args()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    with torch.no_grad():
        (bench_time if args.mode == 'time' else bench_profile)(args, emit)
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
