#!/usr/bin/env python3
"""Device time of the training batch resize, per batch, with HIP events over many batches:
  per_image     today's unaugmented path (BatchLoader._resize_each): zeroed batch tensors, then one image launch and one mask launch per
                example (mrcnn_image_resize_u8_f32, mrcnn_mask_resize_nearest_u8)
  batched       the augmented path's two launches (mrcnn_image_resize_batch_u8_f32, mrcnn_mask_resize_batch_nearest_u8), flip off, the
                same output sizes
  batched_aug   the same kernels with flip on for every other example and scale jitter (short side drawn from --min-sizes, long side
                capped at --max-size), a fresh draw per batch
Batch size 2, COCO-like sources (640 x 480 / 427 x 640, --gt instances each), outputs up to 1024 px; sources already on the device
(the host-to-device copies are the same bytes in all three cases).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def out_size(H, W, min_size, max_size):
    scale = min_size / min(H, W)
    if scale * max(H, W) > max_size:
        scale = max_size / max(H, W)
    return int(H * scale), int(W * scale)


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--gt', type=int, default=8)
    p.add_argument('--min-size', type=int, default=800)
    p.add_argument('--min-sizes', type=int, nargs='+', default=[640, 672, 704, 736, 768, 800])
    p.add_argument('--max-size', type=int, default=1024)
    a = p.parse_args()
    from chainer_maskrcnn._hip import check, lib, ops, ptr
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench.py needs a HIP device')
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    srcs = [(480, 640), (640, 427)]
    imgs = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in srcs]
    masks = [(rs.rand(a.gt, H, W) > 0.5).astype(np.uint8) for H, W in srcs]
    img_d = [torch.from_numpy(x).to(dev) for x in imgs]
    mask_d = [torch.from_numpy(x).to(dev) for x in masks]
    img_pack = torch.from_numpy(np.concatenate([x.reshape(-1) for x in imgs])).to(dev)
    mask_pack = torch.from_numpy(np.concatenate([x.reshape(-1) for x in masks])).to(dev)
    img_offs = np.cumsum([0] + [x.nbytes for x in imgs])[:-1]
    mask_offs = np.cumsum([0] + [x.nbytes for x in masks])[:-1]
    N, G = len(srcs), a.gt

    def geometry(min_sizes, flips):
        outs = [out_size(H, W, m, a.max_size) for (H, W), m in zip(srcs, min_sizes)]
        Hp = -(-max(o[0] for o in outs) // 64) * 64
        Wp = -(-max(o[1] for o in outs) // 64) * 64
        d = ops.resize_descs([(o, H, W, oh, ow, f, 0) for o, (H, W), (oh, ow), f in zip(img_offs, srcs, outs, flips)])
        md = ops.resize_descs([(o, H, W, oh, ow, f, G) for o, (H, W), (oh, ow), f in zip(mask_offs, srcs, outs, flips)])
        return outs, Hp, Wp, d, md

    fixed = geometry([a.min_size] * N, [0] * N)

    def per_image():
        outs, Hp, Wp, _, _ = fixed
        st = torch.cuda.current_stream().cuda_stream
        im = torch.zeros((N, 3, Hp, Wp), dtype=torch.float32, device=dev)
        mk = torch.zeros((N, G, Hp, Wp), dtype=torch.uint8, device=dev)
        for i, ((H, W), (oh, ow)) in enumerate(zip(srcs, outs)):
            check(lib().mrcnn_image_resize_u8_f32(ptr(img_d[i]), H, W, ptr(im[i]), oh, ow, Hp, Wp, 255.0, st))
            check(lib().mrcnn_mask_resize_nearest_u8(ptr(mask_d[i]), G, H, W, ptr(mk[i]), oh, ow, Hp, Wp, st))
        return im, mk

    def batched(geo):
        _, Hp, Wp, d, md = geo
        return ops.image_resize_batch_u8(img_pack, d, Hp, Wp, 255.0), ops.mask_resize_batch_u8(mask_pack, md, G, Hp, Wp)

    drs = np.random.RandomState(1)
    aug_geos = [geometry([int(drs.choice(a.min_sizes)) for _ in range(N)], [(b + i) % 2 for i in range(N)]) for b in range(a.batches)]

    # same bits: the batched kernels with flip off against the per-image path
    x, y = per_image(), batched(fixed)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), 'batched kernels differ from the per-image kernels'

    def timed(fn, n):
        for i in range(a.warmup):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    res = {}
    for rep in range(2):                 # alternate the cases twice: the spread between repeats shows the noise
        res.setdefault('per_image_ms', []).append(timed(lambda i: per_image(), a.batches))
        res.setdefault('batched_ms', []).append(timed(lambda i: batched(fixed), a.batches))
        res.setdefault('batched_aug_ms', []).append(timed(lambda i: batched(aug_geos[i % len(aug_geos)]), a.batches))
    outs, Hp, Wp = fixed[:3]
    written = N * Hp * Wp * (3 * 4 + G)
    line = {'metric': 'ms per bs-2 batch resize (device time, HIP events)', 'batches': a.batches, 'gt_per_image': G,
            'sources': srcs, 'out_sizes': outs, 'padded': (Hp, Wp), 'bytes_written_per_batch': written,
            'per_image_ms': [round(v, 4) for v in res['per_image_ms']], 'batched_ms': [round(v, 4) for v in res['batched_ms']],
            'batched_aug_ms': [round(v, 4) for v in res['batched_aug_ms']],
            'batched_GBps': round(written / (min(res['batched_ms']) * 1e-3) / 1e9, 1),
            'aug_min_sizes': a.min_sizes, 'max_size': a.max_size}
    print(json.dumps(line))


if __name__ == '__main__':
    main()
