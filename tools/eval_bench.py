#!/usr/bin/env python3
"""Cost of validation mAP (chainer_maskrcnn/evaluator.py) on the device.

1. mrcnn_mask_iou_counts_u8 (ops.mask_iou_counts) for (D, G) = (100, 20) at 480x640, 375x500 and 1024x1024, labels off and on:
   time per call from HIP events around `--iters` back-to-back calls (after `--warmup`), and the pack pass alone (the same call
   with G = 0 masks on the other side: zero + pack, no AND-popcount) as a share of 8 TB/s HBM for the bytes it moves.
2. ChainerCV's NumPy mask_iou (a bitwise_and / bitwise_or sum per pair) on the same masks, host clock, for context.
3. The streaming evaluator against predict() alone, per image, on one configuration (the full network, random weights, synthetic
   480x640 images, the evaluate preset); random weights give few detections, so the evaluator's own cost is also timed with
   fixed device-resident predictions of `--fixed-detections` masks per image.

Prints one JSON object per measurement; `--out FILE` also writes them there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X HBM3E


def _masks(rs, D, H, W):
    """Instance-like masks: one filled rectangle each (5..60 % of each side), at random places."""
    m = np.zeros((D, H, W), dtype=bool)
    for d in range(D):
        h, w = int(H * rs.uniform(.05, .6)) + 1, int(W * rs.uniform(.05, .6)) + 1
        y, x = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        m[d, y:y + h, x:x + w] = True
    return m


def _event_time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / iters


def bench_counts(args, emit):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(0)
    D, G = 100, 20
    for H, W in ((480, 640), (375, 500), (1024, 1024)):
        a_np, b_np = _masks(rs, D, H, W), _masks(rs, G, H, W)
        a, b = torch.from_numpy(a_np).cuda(), torch.from_numpy(b_np).cuda()
        la, lb = torch.from_numpy(rs.randint(0, 80, D).astype(np.int32)).cuda(), torch.from_numpy(rs.randint(0, 80, G).astype(np.int32)).cuda()
        HW, NW = H * W, (H * W + 63) // 64
        none = torch.zeros((0, H, W), dtype=torch.bool, device='cuda')
        ab = torch.cat((a, b))
        t_pack = _event_time(lambda: ops.mask_iou_counts(ab, none), args.warmup, args.iters)        # zero + pack of all D + G masks
        pack_bytes = (D + G) * HW + (D + G) * NW * 8             # read one byte per pixel, write one bit per pixel
        for labels in (False, True):
            fn = (lambda: ops.mask_iou_counts(a, b, la, lb)) if labels else (lambda: ops.mask_iou_counts(a, b))
            t = _event_time(fn, args.warmup, args.iters)
            same = int((la[:, None] == lb[None, :]).sum()) if labels else D * G
            call_bytes = pack_bytes + (D + G) * NW * 8            # + the packed words read back (at least once) by the AND-popcount
            emit({'what': 'mask_iou_counts', 'D': D, 'G': G, 'H': H, 'W': W, 'labels': labels, 'same_label_pairs': same,
                  'us_per_call': t * 1e6, 'bytes_per_call': call_bytes, 'call_TBps': call_bytes / t / 1e12,
                  'pack_us': t_pack * 1e6, 'pack_bytes': pack_bytes, 'pack_share_of_hbm_peak': pack_bytes / t_pack / HBM_PEAK})
        if args.numpy:
            t0 = time.perf_counter()
            inter = np.empty((D, G), np.float32)
            for i in range(D):
                for j in range(G):
                    inter[i, j] = np.bitwise_and(a_np[i], b_np[j]).sum() / np.bitwise_or(a_np[i], b_np[j]).sum()
            emit({'what': 'numpy_mask_iou', 'D': D, 'G': G, 'H': H, 'W': W, 'ms_per_call': (time.perf_counter() - t0) * 1e3})


class _FixedTarget(object):
    """predict() returns the same device-resident (D, H, W) masks, labels and scores for every image: the evaluator's own cost."""

    def __init__(self, masks, labels, scores):
        self.out, self.train, self.device = ([masks], [labels], [scores]), True, masks.device

    def predict(self, imgs):
        return self.out


def bench_evaluator(args, emit):
    from chainer_maskrcnn.evaluator import InstanceSegmentationVOCEvaluator, SyntheticEvalDataset
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    H, W = args.image_size
    m = MaskRCNN(n_fg_class=80, device='cuda:0', seed=0)
    m.use_preset('evaluate')
    m.score_thresh = args.score_thresh
    data = SyntheticEvalDataset(args.images, H, W, n_fg_class=80)
    examples = [data[i] for i in range(len(data))]
    imgs = [torch.from_numpy(e[0]) for e in examples]

    def per_image(fn):
        fn()                                                    # warm-up of every shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(imgs), r

    t_pred, (_, labels, _) = per_image(lambda: m.predict(imgs))
    t_eval, r = per_image(lambda: InstanceSegmentationVOCEvaluator(examples, m).evaluate())
    emit({'what': 'evaluator_vs_predict', 'image': [H, W], 'images': len(imgs), 'score_thresh': m.score_thresh,
          'detections_per_image': float(np.mean([int(l.shape[0]) for l in labels])), 'gt_per_image': 8,
          'predict_ms_per_image': t_pred * 1e3, 'evaluate_ms_per_image': t_eval * 1e3,
          'overhead_fraction_of_predict': (t_eval - t_pred) / t_pred, 'map': r['main/map']})
    # the evaluator alone with D detections per image (random weights give few): fixed device-resident predictions
    rs = np.random.RandomState(1)
    D = args.fixed_detections
    fixed = _FixedTarget(torch.from_numpy(_masks(rs, D, H, W)).cuda(), torch.from_numpy(rs.randint(0, 80, D).astype(np.int32)).cuda(),
                         torch.from_numpy(rs.rand(D).astype(np.float32)).cuda())
    t_fixed, _ = per_image(lambda: InstanceSegmentationVOCEvaluator(examples, fixed).evaluate())
    emit({'what': 'evaluator_own_cost', 'image': [H, W], 'images': len(imgs), 'detections_per_image': D, 'gt_per_image': 8,
          'evaluator_ms_per_image': t_fixed * 1e3, 'fraction_of_predict': t_fixed / t_pred})


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--numpy', type=int, default=1, help='also time the NumPy mask_iou (seconds per shape)')
    p.add_argument('--images', type=int, default=8)
    p.add_argument('--image-size', type=int, nargs=2, default=[480, 640])
    p.add_argument('--score-thresh', type=float, default=0.05, help='predict() threshold (the evaluate preset: 0.05)')
    p.add_argument('--fixed-detections', type=int, default=100)
    p.add_argument('--evaluator', type=int, default=1, help='0: the mask_iou_counts part only')
    p.add_argument('--out', default='')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_bench.py measures on a HIP device; none is visible')
    out = open(args.out, 'w') if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()
    bench_counts(args, emit)
    if args.evaluator:
        bench_evaluator(args, emit)


if __name__ == '__main__':
    main()
