#!/usr/bin/env python3
"""Device time of the large-scale-jitter batch assembly, per batch, with HIP events over many batches:
  pair      the yardstick: the batched flip / jitter pair (mrcnn_image_resize_batch_u8_f32, mrcnn_mask_resize_batch_nearest_u8) writing the
            same S x S canvas, the sources resized to fill it (longer side S), every other example mirrored
  lsj_s1    the LSJ launches at s = 1 (the same resized sizes, no crop)
  lsj_s2    at s = 2, the S x S window at an interior offset of the 2S virtual resize
  lsj_s01   at s = 0.1: the image is a tenth of the canvas, the rest is padding
For each LSJ case the stages are timed on their own - image writer, box / compaction launches (one fill, reduce, finalize), mask writer -
and together, as the loader issues them.  Batch size 2, the sources and instance masks of augment_bench.py (640 x 480 / 427 x 640,
--gt instances each), S = 1024; sources already on the device.  Two alternating repeats in one process: the spread between them shows
the noise.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_TBPS = 8.0         # HBM3E peak of the MI355X


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--gt', type=int, default=8)
    p.add_argument('--size', type=int, default=1024)
    a = p.parse_args()
    from chainer_maskrcnn._hip import ops
    from chainer_maskrcnn.dataset.augment import lsj_geometry
    if not torch.cuda.is_available():
        raise SystemExit('lsj_bench.py needs a HIP device')
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    srcs = [(480, 640), (640, 427)]
    imgs = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in srcs]
    masks = [(rs.rand(a.gt, H, W) > 0.5).astype(np.uint8) for H, W in srcs]
    img_pack = torch.from_numpy(np.concatenate([x.reshape(-1) for x in imgs])).to(dev)
    mask_pack = torch.from_numpy(np.concatenate([x.reshape(-1) for x in masks])).to(dev)
    img_offs = np.cumsum([0] + [x.nbytes for x in imgs])[:-1]
    mask_offs = np.cumsum([0] + [x.nbytes for x in masks])[:-1]
    N, G, S = len(srcs), a.gt, a.size
    flips = [i % 2 for i in range(N)]
    labels_in = torch.arange(N * G, dtype=torch.int32, device=dev).reshape(N, G)

    def lsj_descs(s, u):
        geos = [lsj_geometry(H, W, S, s, u, u) for H, W in srcs]
        d = ops.crop_descs([(o, H, W, g[0], g[1], f, 0) + g[2:] for o, (H, W), g, f in zip(img_offs, srcs, geos, flips)])
        md = ops.crop_descs([(o, H, W, g[0], g[1], f, G) + g[2:] for o, (H, W), g, f in zip(mask_offs, srcs, geos, flips)])
        return geos, d, md

    fill = [lsj_geometry(H, W, S, 1.0, 0.0, 0.0)[:2] for H, W in srcs]
    pair_d = ops.resize_descs([(o, H, W, oh, ow, f, 0) for o, (H, W), (oh, ow), f in zip(img_offs, srcs, fill, flips)])
    pair_md = ops.resize_descs([(o, H, W, oh, ow, f, G) for o, (H, W), (oh, ow), f in zip(mask_offs, srcs, fill, flips)])
    cases = {'lsj_s1': lsj_descs(1.0, 0.5), 'lsj_s2': lsj_descs(2.0, 0.5), 'lsj_s01': lsj_descs(0.1, 0.5)}
    gathers = {k: ops.mask_crop_boxes_u8(mask_pack, md, labels_in, G, S, S)[2] for k, (_, _, md) in cases.items()}

    def pair():
        return ops.image_resize_batch_u8(img_pack, pair_d, S, S, 255.0), ops.mask_resize_batch_u8(mask_pack, pair_md, G, S, S)

    def stages(k):
        _, d, md = cases[k]
        return {'image': lambda: ops.image_resize_crop_batch_u8(img_pack, d, S, S, 255.0),
                'boxes': lambda: ops.mask_crop_boxes_u8(mask_pack, md, labels_in, G, S, S),
                'masks': lambda: ops.mask_resize_crop_batch_u8(mask_pack, md, gathers[k], S, S),
                'all': lambda: (ops.image_resize_crop_batch_u8(img_pack, d, S, S, 255.0),
                                ops.mask_resize_crop_batch_u8(mask_pack, md, ops.mask_crop_boxes_u8(mask_pack, md, labels_in, G, S, S)[2], S, S))}

    # same bits: s = 1 leaves the window at (0, 0) and nothing is dropped, so the LSJ writers must reproduce the pair
    x, y = pair(), stages('lsj_s1')['all']()
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), 'the LSJ writers at s = 1 differ from the batched pair'

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batches

    res = {}
    for rep in range(2):
        res.setdefault('pair_ms', []).append(timed(pair))
        for k in cases:
            for stage, fn in stages(k).items():
                res.setdefault('%s_%s_ms' % (k, stage), []).append(timed(fn))
    written = N * S * S * (3 * 4 + G)
    line = {'metric': 'ms per bs-2 batch (device time, HIP events)', 'batches': a.batches, 'gt_per_image': G, 'sources': srcs, 'canvas': S,
            'geometry': {k: [list(g) for g in v[0]] for k, v in cases.items()}, 'kept': {k: int((g >= 0).sum()) for k, g in gathers.items()},
            'bytes_written_per_batch': written, 'box_pass_samples_per_batch': {k: int(sum(G * g[4] * g[5] for g in v[0])) for k, v in cases.items()}}
    line.update({k: [round(t, 4) for t in v] for k, v in res.items()})
    writers = {'pair': min(res['pair_ms'])}
    writers.update({k: min(res[k + '_image_ms']) + min(res[k + '_masks_ms']) for k in cases})
    line['writers_TBps'] = {k: round(written / (t * 1e-3) / 1e12, 3) for k, t in writers.items()}
    line['writers_share_of_%g_TBps_peak' % PEAK_TBPS] = {k: round(written / (t * 1e-3) / 1e12 / PEAK_TBPS, 3) for k, t in writers.items()}
    print(json.dumps(line))


if __name__ == '__main__':
    main()
