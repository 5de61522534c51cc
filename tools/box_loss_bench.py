#!/usr/bin/env python3
"""What the IoU box regression losses cost on the device, measured in ONE process with the variants interleaved:
  kernels   device time (HIP events, median of --reps windows of 20 calls) of mrcnn_box_iou_loss_f32 - loss and gradient, its three
            launches - for giou, diou and ciou, beside mrcnn_smooth_l1_f32 on the same buffers, at the two shapes of the training step:
              head  M = 1024 rows of the head's box_out buffer (ldx = out_p = 96, the loc columns at LOC0 = 88, gfill = 8), a quarter of
                    the rows positive, roi_period = M
              rpn   M = 2 A rows of 4 (A = the anchors of a --size x --size image: 261888 at 1024), about 1 % positive, the anchors
                    shared by the two images (roi_period = A)
            These calls are latency-bound (a few launches over little data; the RPN's gradient pass is a zero-fill of 8 MB), so the table
            gives times, not a fraction of the HBM rate.
  step      the bs-2 --size x --size mask training step with box_loss = rpn_box_loss = smooth_l1 and = giou, two trainers in one process,
            windows alternating: step time (device events, median).  The trainers share their auxiliary and step streams, as in
            tools/groupnorm_bench.py.
Prints one JSON object.

usage: box_loss_bench.py [--steps 10] [--reps 5] [--size 1024] [--skip-step 0] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

KINDS = ('giou', 'diou', 'ciou')


def _event_ms(fn, n):
    """Milliseconds per call of fn over n back-to-back calls, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _boxes(rs, n, size):
    side = rs.uniform(16.0, size / 2.0, (n, 2))
    tl = rs.uniform(0.0, size - side)
    return np.concatenate([tl, tl + side], 1).astype(np.float32)


def kernel_table(args, dev):
    from chainer_maskrcnn._hip import ops
    A = 3 * sum((args.size // s) ** 2 for s in (4, 8, 16, 32, 64))
    shapes = [('head', 1024, 96, 88, 8, 1024, 0.25, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)),
              ('rpn', 2 * A, 4, 0, 0, A, 0.01, (0., 0., 0., 0.), (1., 1., 1., 1.))]
    rows = []
    for name, M, ldx, col0, gfill, period, p_pos, mean, std in shapes:
        rs = np.random.RandomState(M)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        t = (rs.standard_normal((M, 4)) * (0.3 / np.asarray(std))).astype(np.float32)
        buf = rs.standard_normal((M, ldx)).astype(np.float32)
        buf[:, col0:col0 + 4] = t + (rs.standard_normal((M, 4)) * (0.2 / np.asarray(std))).astype(np.float32)
        label = np.where(rs.rand(M) < p_pos, 1, np.where(rs.rand(M) < 0.5, 0, -1)).astype(np.int32)
        x, t, rois, label = d(buf), d(t), d(_boxes(rs, period, args.size)), d(label)
        gx, out = torch.empty_like(x), torch.empty((2,), device=dev)
        cases = [('smooth_l1', lambda i: ops.smooth_l1(x, ldx, t, label, M, 1.0, gfill=gfill, col0=col0, gx=gx, out=out))]
        for kind in KINDS:
            cases.append((kind, lambda i, kind=kind: ops.box_iou_loss(x, ldx, t, rois, label, M, kind, mean, std, roi_period=period,
                                                                      gfill=gfill, col0=col0, gx=gx, out=out)))
        us = {n_: [] for n_, _ in cases}
        for _, fn in cases:
            _event_ms(fn, 5)
        for _ in range(args.reps):
            for n_, fn in cases:
                us[n_].append(_event_ms(fn, 20) * 1e3)
        for n_, _ in cases:
            rows.append({'shape': name, 'M': M, 'ldx': ldx, 'col0': col0, 'gfill': gfill, 'roi_period': period,
                         'positive_rows': int((label > 0).sum()), 'loss': n_, 'launches': 3, 'us_median': round(statistics.median(us[n_]), 2),
                         'us_all': [round(v, 2) for v in us[n_]]})
    return rows


def step_table(args, dev):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay
    from chainer_maskrcnn.utils.synthetic import make_batch
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    variants = {}
    for name in ('smooth_l1', 'giou'):
        model = MaskRCNN(n_fg_class=80, device=dev)
        chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic='bf16x6_behind_backbone',
                                      box_loss=name, rpn_box_loss=name)
        opt = MomentumSGD(lr=1e-4).setup(chain)
        opt.add_hook(WeightDecay(5e-4))
        if variants:                    # one set of streams for both trainers (tools/groupnorm_bench.py)
            first_opt, first_chain = next(iter(variants.values()))
            chain._aux, opt._hi = first_chain._aux, first_opt._hi
        variants[name] = (opt, chain)
    for opt, chain in variants.values():
        for _ in range(5):
            opt.update(chain, *batch, 1.0)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    finite = {}
    for _ in range(args.reps):
        for name, (opt, chain) in variants.items():
            opt.update(chain, *batch, 1.0)          # the variant's first step after the switch is not timed
            torch.cuda.synchronize()
            ms[name].append(_event_ms(lambda i: opt.update(chain, *batch, 1.0), args.steps))
            finite[name] = bool(torch.isfinite(chain.observation['loss']).item())
    base = statistics.median(ms['smooth_l1'])
    return [{'box_loss': name, 'rpn_box_loss': name, 'step_ms_median': round(statistics.median(ms[name]), 3),
             'step_ms_all': [round(v, 3) for v in ms[name]], 'vs_smooth_l1': round(statistics.median(ms[name]) / base, 4),
             'images_per_s': round(2000.0 / statistics.median(ms[name]), 2), 'loss_finite': finite[name]} for name in variants]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10, help='steps per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--skip-step', type=int, default=0, choices=[0, 1], help='1: the kernel table only')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('box_loss_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(dev), 'size': args.size, 'batch': 2, 'kernels': kernel_table(args, dev)}
    if not args.skip_step:
        res['step'] = step_table(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
