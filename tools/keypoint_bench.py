#!/usr/bin/env python3
"""Cost of keypoint inference and COCO keypoint AP (chainer_maskrcnn/evaluator.py KeypointCOCOEvaluator) on the device.

1. mrcnn_keypoint_decode_f32 (ops.keypoint_decode) at D = 1, 20, 100 detections, K = 17, S = 56, Cp = 32: time per call from HIP
   events around `--iters` back-to-back calls (after `--warmup`), with the bytes it reads (algorithmic D*S^2*K*4, moved D*S^2*Cp*4)
   as a share of 8 TB/s; the same decode as a torch expression (permute + argmax + logsumexp) on the same tensors, for context.
   Kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script.
2. The evaluator's own cost per image with a fixed stand-in for predict_keypoints (`--fixed-detections` device-resident detections
   per image), as tools/eval_bench.py does for the mask evaluator.

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


def _torch_decode(heat, bbox, K):
    """The same outputs as keypoint_decode in torch (for context only): argmax, logit, softmax at the argmax, cell corner in the box."""
    D, S = heat.shape[0], heat.shape[1]
    h = heat[..., :K].permute(0, 3, 1, 2).reshape(D, K, S * S)
    logit, idx = h.max(-1)
    prob = torch.exp(logit - torch.logsumexp(h, -1))
    y = (idx // S).float() * ((bbox[:, 2:3] - bbox[:, 0:1]) / S) + bbox[:, 0:1]
    x = (idx % S).float() * ((bbox[:, 3:4] - bbox[:, 1:2]) / S) + bbox[:, 1:2]
    return torch.stack((y, x, logit, prob), -1)


def bench_decode(args, emit):
    from chainer_maskrcnn._hip import ops
    rs = np.random.RandomState(0)
    S, Cp, K = 56, 32, 17
    for D in (1, 20, 100):
        heat = torch.from_numpy(rs.standard_normal((D, S, S, Cp)).astype(np.float32)).cuda()
        y0, x0 = rs.uniform(0, 400, D), rs.uniform(0, 500, D)
        bbox = torch.from_numpy(np.stack([y0, x0, y0 + rs.uniform(20, 300, D), x0 + rs.uniform(20, 300, D)], 1).astype(np.float32)).cuda()
        t = _event_time(lambda: ops.keypoint_decode(heat, bbox, K), args.warmup, args.iters)
        t_torch = _event_time(lambda: _torch_decode(heat, bbox, K), args.warmup, args.iters)
        alg, moved = D * S * S * K * 4, D * S * S * Cp * 4
        emit({'what': 'keypoint_decode', 'D': D, 'K': K, 'S': S, 'Cp': Cp, 'us_per_call': t * 1e6, 'algorithmic_bytes': alg,
              'moved_bytes': moved, 'moved_share_of_hbm_peak': moved / t / HBM_PEAK, 'torch_us_per_call': t_torch * 1e6})


class _FixedTarget(object):
    """predict_keypoints() returns the same device-resident (D, K, 4) keypoints and scores for every image: the evaluator's own cost."""

    def __init__(self, kp, scores):
        self.out, self.train, self.device = ([kp], [torch.zeros_like(scores, dtype=torch.int32)], [scores]), True, kp.device

    def predict_keypoints(self, imgs):
        return self.out


def bench_evaluator(args, emit):
    from chainer_maskrcnn.evaluator import KeypointCOCOEvaluator, SyntheticKeypointEvalDataset
    H, W = args.image_size
    data = SyntheticKeypointEvalDataset(args.images, H, W)
    examples = [data[i] for i in range(len(data))]
    rs = np.random.RandomState(1)
    D = args.fixed_detections
    kp = np.zeros((D, 17, 4), np.float32)
    kp[..., 0], kp[..., 1] = rs.uniform(0, H, (D, 17)), rs.uniform(0, W, (D, 17))
    fixed = _FixedTarget(torch.from_numpy(kp).cuda(), torch.from_numpy(rs.rand(D).astype(np.float32)).cuda())
    ev = KeypointCOCOEvaluator(examples, fixed)
    ev.evaluate()                                               # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ev.evaluate()
    torch.cuda.synchronize()
    emit({'what': 'keypoint_evaluator_own_cost', 'image': [H, W], 'images': len(examples), 'detections_per_image': D, 'gt_per_image': 8,
          'evaluator_ms_per_image': (time.perf_counter() - t0) / len(examples) * 1e3, 'map': r['main/map']})


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--iters', type=int, default=100)
    p.add_argument('--images', type=int, default=16)
    p.add_argument('--image-size', type=int, nargs=2, default=[480, 640])
    p.add_argument('--fixed-detections', type=int, default=100)
    p.add_argument('--evaluator', type=int, default=1, help='0: the decode part only')
    p.add_argument('--out', default='')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('keypoint_bench.py measures on a HIP device; none is visible')
    out = open(args.out, 'w') if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()
    bench_decode(args, emit)
    if args.evaluator:
        bench_evaluator(args, emit)


if __name__ == '__main__':
    main()
