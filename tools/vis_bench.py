#!/usr/bin/env python3
"""Cost of drawing detections on the device (csrc/vis.hip, chainer_maskrcnn/vis.py) against what it replaces.

Per shape - D in --detections (10, 100) at every --sizes (800 x 1333, 480 x 640) - on a seeded scene (box-shaped masks with holes,
their boxes, class colours, the labels' primitives from vis.instance_primitives, everything drawn):
  render_ms      device time of one mrcnn_vis_render_u8 launch, inputs resident: HIP events around each of --iters calls after --warmup,
                 the median (min and max with it)
  bytes_moved    what the kernel must move: D * H * W mask bytes + 12 * H * W image bytes + 3 * H * W picture bytes; gb_per_s =
                 bytes_moved / render_ms and its share of the 8 TB/s HBM peak: a plausibility check, not a kernel's share of peak (halo
                 rows are read twice, mostly from L2)
  copy_ms        the (D,H,W) mask tensor device -> host alone (torch .cpu(), host clock around a synchronise), the median of --copies:
                 what compositing on the host would pay before it starts
  numpy_ms       the NumPy restatement (tests/vis_reference.py) on the same inputs, one run; its picture must equal the device's
Prints one JSON object per shape; --out FILE also writes them."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8e12


def scene(seed, D, H, W):
    from chainer_maskrcnn import vis
    rs = np.random.RandomState(seed)
    img = (rs.rand(3, H, W) * 255).astype(np.float32)
    masks = np.zeros((D, H, W), np.uint8)
    bbox = np.zeros((D, 4), np.float32)
    for d in range(D):
        h, w = rs.randint(H // 8, H // 2), rs.randint(W // 8, W // 2)
        y, x = rs.randint(0, H - h), rs.randint(0, W - w)
        masks[d, y:y + h, x:x + w] = rs.rand(h, w) < 0.98
        bbox[d] = [y, x, y + h, x + w]
    labels, scores = rs.randint(0, 80, D), rs.rand(D).astype(np.float32)
    order, colors, prims = vis.instance_primitives(H, W, bbox, labels, scores, None, 'class', True, 1)
    return img, masks, bbox, colors, order, prims


def bench_shape(D, H, W, args):
    import vis_reference as ref
    from chainer_maskrcnn import _hip, vis
    from chainer_maskrcnn._hip import ops
    img, masks, bbox, colors, order, prims = scene(D * 7 + H, D, H, W)
    dev = 'cuda:0'
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_img, t_masks, t_bbox, t_colors, t_order = up(img), up(masks), up(bbox), up(colors), up(order)
    t_prims, t_font = up(prims.view(np.int32).reshape(-1, 8)), up(vis.FONT.view(np.int64))
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    flags = ops.VIS_DRAW_MASKS | ops.VIS_DRAW_CONTOURS | ops.VIS_DRAW_BOXES
    lib, p = _hip.lib(), _hip.ptr

    def launch():
        _hip.check(lib.mrcnn_vis_render_u8(p(t_img), H, W, p(t_masks), p(t_bbox), p(t_colors), p(t_order), D, 128, 2, flags, p(t_prims),
                                           len(prims), p(t_font), len(vis.FONT), p(out), _hip.stream_ptr()))
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    copies = []
    for _ in range(args.copies):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = t_masks.cpu()
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    del host
    t0 = time.perf_counter()
    want = ref.render(img, masks, bbox, colors, order, 128, 2, flags, prims, vis.FONT)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(out.cpu().numpy(), want))
    if not same:
        raise RuntimeError('the device picture differs from the NumPy restatement at D %d, %d x %d' % (D, H, W))
    moved = D * H * W + 15 * H * W
    med = float(np.median(ms))
    return {'D': D, 'H': H, 'W': W, 'primitives': int(len(prims)), 'render_ms': round(med, 4), 'render_ms_min': round(min(ms), 4),
            'render_ms_max': round(max(ms), 4), 'iters': args.iters, 'bytes_moved': moved, 'gb_per_s': round(moved / med / 1e6, 1),
            'share_of_8TBps': round(moved / (med * 1e-3) / HBM_PEAK, 4), 'copy_ms': round(float(np.median(copies)), 3),
            'numpy_ms': round(numpy_ms, 1), 'equal_to_numpy': same}


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--detections', type=int, nargs='+', default=[10, 100])
    p.add_argument('--sizes', type=int, nargs='+', default=[800, 1333, 480, 640], help='H W pairs')
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--copies', type=int, default=5)
    p.add_argument('--out', default='')
    args = p.parse_args()
    if len(args.sizes) % 2:
        raise ValueError('--sizes takes H W pairs')
    if not torch.cuda.is_available():
        raise RuntimeError('tools/vis_bench.py measures on a HIP device; none is available')
    rows = []
    for H, W in zip(args.sizes[::2], args.sizes[1::2]):
        for D in args.detections:
            rows.append(bench_shape(D, H, W, args))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
