#!/usr/bin/env python3
"""Cost of COCO box / mask AP and results export (chainer_maskrcnn/evaluator.py InstanceSegmentationCOCOEvaluator) on the device.

1. mrcnn_mask_rle_count_u8 + mrcnn_mask_rle_write_u8 (ops.mask_rle_encode) at D = 100 for masks from mask_paste and for random
   masks (noise, the most runs), at 375x500, 480x640 and 1024x1024: time per call from HIP events around `--iters` back-to-back
   calls (after `--warmup`; the call includes its one device->host read of the run total) and with the copy of offsets and counts to
   the host that the evaluator makes.  Bytes each tile pass reads (every mask byte once) are printed for the share of 8 TB/s; the
   kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
2. The host alternative: copy the masks to the host, then dataset.coco_api.rle_encode (NumPy) per mask.
3. The evaluator's own cost per image with `--fixed-detections` device-resident detections and 8 ground truths (a fixed stand-in for
   predict, 480x640 synthetic images), without and with export, and the host matching alone.

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


def _pasted(rs, D, H, W):
    from chainer_maskrcnn._hip import ops
    S, Cm = 28, 81
    logits = torch.from_numpy(rs.standard_normal((D, S, S, Cm)).astype(np.float32) * 3).cuda()
    h, w = H * rs.uniform(.05, .6, D) + 1, W * rs.uniform(.05, .6, D) + 1
    y0, x0 = rs.uniform(0, 1, D) * (H - h), rs.uniform(0, 1, D) * (W - w)
    bbox = np.stack([y0, x0, y0 + h, x0 + w], 1).astype(np.float32)
    label = rs.randint(0, 80, D).astype(np.int32)
    return ops.mask_paste(logits, torch.from_numpy(label).cuda(), torch.from_numpy(bbox).cuda(), (H, W)).bool()


def bench_encode(args, emit):
    from chainer_maskrcnn._hip import ops
    from chainer_maskrcnn.dataset.coco_api import rle_encode
    rs = np.random.RandomState(0)
    D = 100
    for H, W in ((375, 500), (480, 640), (1024, 1024)):
        for kind in ('mask_paste', 'random'):
            m = _pasted(rs, D, H, W) if kind == 'mask_paste' else torch.from_numpy(rs.rand(D, H, W) < 0.5).cuda()
            offsets, counts, _ = ops.mask_rle_encode(m)
            runs = int(counts.shape[0])
            t = _event_time(lambda: ops.mask_rle_encode(m), args.warmup, args.iters)
            t_copy = _event_time(lambda: [x.cpu() for x in ops.mask_rle_encode(m)[:2]], args.warmup, args.iters)
            n_seg = D * W * ((H + 63) // 64)
            emit({'what': 'mask_rle_encode', 'kind': kind, 'D': D, 'H': H, 'W': W, 'runs': runs, 'us_per_call': t * 1e6,
                  'us_per_call_with_copy': t_copy * 1e6, 'mask_bytes_per_pass': D * H * W, 'segment_bytes': n_seg * 8,
                  'counts_bytes': runs * 4, 'call_share_of_hbm_peak': 2 * D * H * W / t / HBM_PEAK})
            if args.numpy:
                def host():
                    mh = m.cpu().numpy()
                    return [rle_encode(mh[d]) for d in range(D)]
                host()
                t0 = time.perf_counter()
                for _ in range(args.numpy):
                    host()
                t_host = (time.perf_counter() - t0) / args.numpy
                emit({'what': 'host_encode', 'kind': kind, 'D': D, 'H': H, 'W': W, 'ms_per_call': t_host * 1e3,
                      'device_speedup_with_copy': t_host / t_copy})


class _FixedTarget(object):
    """predict() returns the same device-resident masks, labels, scores and boxes for every image: the evaluator's own cost."""

    def __init__(self, masks, labels, scores, boxes):
        self.out, self.train, self.device = ([masks], [labels], [scores]), True, masks.device
        self.last_bboxes = [boxes]

    def predict(self, imgs):
        return self.out


def bench_evaluator(args, emit):
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, SyntheticCOCOEvalDataset
    H, W = args.image_size
    data = SyntheticCOCOEvalDataset(args.images, H, W, n_fg_class=80)
    examples = [data[i] for i in range(len(data))]
    rs = np.random.RandomState(1)
    D = args.fixed_detections
    m = _pasted(rs, D, H, W)
    ys, xs = rs.uniform(0, H / 2, D), rs.uniform(0, W / 2, D)
    boxes = np.stack([ys, xs, ys + rs.uniform(4, H / 2, D), xs + rs.uniform(4, W / 2, D)], 1).astype(np.float32)
    fixed = _FixedTarget(m, torch.from_numpy(rs.randint(0, 80, D).astype(np.int32)).cuda(), torch.from_numpy(rs.rand(D).astype(np.float32)).cuda(),
                         torch.from_numpy(boxes).cuda())

    def per_image(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(examples)
    t_eval = per_image(lambda: InstanceSegmentationCOCOEvaluator(examples, fixed).evaluate())
    t_export = per_image(lambda: InstanceSegmentationCOCOEvaluator(examples, fixed, results=[]).evaluate())
    # the host matching alone: the accumulators on the IoU matrices the evaluator builds, without the device work
    from chainer_maskrcnn import evaluations
    acc_t = 0.0
    ev = InstanceSegmentationCOCOEvaluator(examples, fixed)
    orig = evaluations.COCOInstanceMatchAccumulator.add_image

    def timed(self, *a, **k):
        nonlocal acc_t
        t0 = time.perf_counter()
        orig(self, *a, **k)
        acc_t += time.perf_counter() - t0
    evaluations.COCOInstanceMatchAccumulator.add_image = timed
    try:
        ev.evaluate()
    finally:
        evaluations.COCOInstanceMatchAccumulator.add_image = orig
    emit({'what': 'evaluator_own_cost', 'image': [H, W], 'images': len(examples), 'detections_per_image': D, 'gt_per_image': 8,
          'evaluate_ms_per_image': t_eval * 1e3, 'evaluate_with_export_ms_per_image': t_export * 1e3,
          'host_matching_ms_per_image': acc_t / len(examples) * 1e3})


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--numpy', type=int, default=2, help='host-alternative repetitions per shape (0: skip)')
    p.add_argument('--images', type=int, default=8)
    p.add_argument('--image-size', type=int, nargs=2, default=[480, 640])
    p.add_argument('--fixed-detections', type=int, default=100)
    p.add_argument('--evaluator', type=int, default=1, help='0: the encoder part only')
    p.add_argument('--out', default='')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('coco_eval_bench.py measures on a HIP device; none is visible')
    out = open(args.out, 'w') if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
    bench_encode(args, emit)
    if args.evaluator:
        bench_evaluator(args, emit)


if __name__ == '__main__':
    main()
