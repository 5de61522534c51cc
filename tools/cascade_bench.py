#!/usr/bin/env python3
"""What Cascade R-CNN box stages cost on the device, measured in ONE process with the variants interleaved:
  kernels   device time (HIP events, median of --reps windows of 20 calls) of mrcnn_cascade_refine_f32 (training form with G = 32 ground-truth
            boxes per image, and the inference form) and mrcnn_cascade_prob_f32 (K = 3, 81 classes) at R = 2 * 512 rows, beside the bytes a
            call must move.  Both are latency-bound (one launch over a thousand rows): the time is that of a launch, not of the bytes.
  step      the bs-2 1024 x 1024 mask training step with the cascade off (the parent commit's step) and on (IoU 0.5 / 0.6 / 0.7), two models in
            one process, windows alternating: step time (device events, median), peak allocated memory of a window and its delta.  The two
            trainers share their auxiliary and step streams, as in tools/groupnorm_bench.py.
Prints one JSON object.

usage: cascade_bench.py [--steps 10] [--reps 5] [--size 1024] [--skip-step 0] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)
import torch  # noqa: E402

N, S, G, K, N_CLASS, LD, LOC0 = 2, 512, 32, 3, 81, 88, 84
IOUS = (0.5, 0.6, 0.7)


def _event_ms(fn, n):
    """Milliseconds per call of fn over n back-to-back calls, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_table(args, dev):
    from chainer_maskrcnn._hip import ops
    from chainer_maskrcnn.model.maskrcnn import CASCADE_STDS
    g = torch.Generator(device='cpu').manual_seed(1)
    rows_n = N * S
    y1, x1 = torch.rand(rows_n, generator=g) * 700, torch.rand(rows_n, generator=g) * 700
    rois = torch.stack([y1, x1, y1 + 20 + torch.rand(rows_n, generator=g) * 300, x1 + 20 + torch.rand(rows_n, generator=g) * 300], 1).to(dev)
    outs = [torch.randn((rows_n, LD), generator=g).to(dev) for _ in range(K)]
    prev = torch.zeros((rows_n,), dtype=torch.int32, device=dev)
    gy, gx = torch.rand((N, G), generator=g) * 700, torch.rand((N, G), generator=g) * 700
    gt = torch.stack([gy, gx, gy + 30 + torch.rand((N, G), generator=g) * 290, gx + 30 + torch.rand((N, G), generator=g) * 290], 2).to(dev).contiguous()
    gl = torch.randint(0, 80, (N, G), generator=g).to(torch.int32).to(dev)
    ng = torch.full((N,), G, dtype=torch.int32, device=dev)
    mean = (0., 0., 0., 0.)

    def train(i):
        ops.cascade_refine(rois, outs[0], LOC0, N, mean, CASCADE_STDS[0], (1024., 1024.), prev_label=prev, gt_boxes=gt, gt_labels=gl, n_gt=ng,
                           iou_thresh=0.6, std_next=CASCADE_STDS[1])

    def infer(i):
        ops.cascade_refine(rois, outs[0], LOC0, N, mean, CASCADE_STDS[0], (1024., 1024.))

    def prob(i):
        ops.cascade_prob(outs, N_CLASS)
    per_row_in, per_row_out = 16 + 16 + 4, 16 + 20 + 4
    cases = [('cascade_refine, training form (G = %d)' % G, rows_n * (per_row_in + per_row_out + 16 + 4 + 4) + N * G * 20 + N * 4, train),
             ('cascade_refine, inference form', rows_n * (per_row_in - 4 + per_row_out), infer),
             ('cascade_prob (K = %d, %d classes)' % (K, N_CLASS), (K + 1) * rows_n * N_CLASS * 4, prob)]
    us = {name: [] for name, _, _ in cases}
    for _, _, fn in cases:
        _event_ms(fn, 5)
    for _ in range(args.reps):
        for name, _, fn in cases:
            us[name].append(_event_ms(fn, 20) * 1e3)
    return [{'call': name, 'rows': rows_n, 'us_median': round(statistics.median(us[name]), 2), 'us_all': [round(v, 2) for v in us[name]],
             'bytes': int(nbytes), 'note': 'through the Python wrapper: output allocation and the ctypes call are in the window'}
            for name, nbytes, _ in cases]


def step_table(args, dev):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay
    from chainer_maskrcnn.utils.synthetic import make_batch
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    variants = {}
    for name, ious in (('off', None), ('on', IOUS)):
        model = MaskRCNN(n_fg_class=80, device=dev, cascade_ious=ious)
        chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic='bf16x6_behind_backbone')
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
    peak = {name: 0 for name in variants}
    finite = {}
    for _ in range(args.reps):
        for name, (opt, chain) in variants.items():
            opt.update(chain, *batch, 1.0)          # the variant's first step after the switch is not timed
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ms[name].append(_event_ms(lambda i: opt.update(chain, *batch, 1.0), args.steps))
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated(dev))
            finite[name] = all(bool(torch.isfinite(v).item()) for v in chain.observation.values())
    base = statistics.median(ms['off'])
    rows = [{'cascade': name, 'step_ms_median': round(statistics.median(ms[name]), 3), 'step_ms_all': [round(v, 3) for v in ms[name]],
             'vs_off': round(statistics.median(ms[name]) / base, 4), 'images_per_s': round(2000.0 / statistics.median(ms[name]), 2),
             'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1), 'losses_finite': finite[name],
             'n_params': variants[name][1].faster_rcnn.ps.n_params()} for name in variants]
    rows[1]['peak_delta_MiB'] = round((peak['on'] - peak['off']) / 2 ** 20, 1)
    rows[1]['note'] = 'both models are resident in both windows: the peak is that of the process, its delta that of the cascade step'
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10, help='steps per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--skip-step', type=int, default=0, choices=[0, 1], help='1: the kernel table only')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cascade_bench.py measures on a HIP device; none found')
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
