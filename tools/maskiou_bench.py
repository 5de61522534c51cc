#!/usr/bin/env python3
"""What Mask Scoring R-CNN costs on the device.  Two parts, each a child process of its own with its own time limit:
  kernels   device time (HIP events, median of --reps windows of 20 calls) of every new kernel at the workload's shape - batch 2, 1024 x 1024
            images, G = 32 mask slots per image of which 20 and 12 are used, the pos_cap = 64 mask rows per image, 256 feature channels,
            80 classes - beside the bytes a call must move at the least.
  step      the bs-2 1024 x 1024 mask training step of bench.py with mask_iou off (the parent commit's step) and on, two models in one
            process, windows alternating: step time (device events, median and range of the windows), peak allocated memory and its delta.
Prints one JSON object; --out also writes it to a file.

usage: maskiou_bench.py [--part all|kernels|step] [--steps 10] [--reps 5] [--size 1024] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)

N, G, N_GT, S, ROWS, C, N_FG, CP = 2, 32, (20, 12), 256, 64, 256, 80, 96
LIMITS = {'kernels': 240, 'step': 480}          # seconds per part


def _event_ms(fn, n):
    """Milliseconds per call of fn over n back-to-back calls, between two device events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_table(args, dev):
    import numpy as np
    import torch
    from chainer_maskrcnn._hip import ops
    H = W = args.size
    rs = np.random.RandomState(1)
    masks = np.zeros((N, G, H, W), np.uint8)
    roi = np.zeros((N * S, 4), np.float32)
    assign = np.zeros((N * S,), np.int32)
    boxes = np.zeros((N, G, 4))
    for i in range(N):
        for g in range(N_GT[i]):
            h, w = rs.randint(H // 16, H // 2), rs.randint(W // 16, W // 2)
            y, x = rs.randint(0, H - h), rs.randint(0, W - w)
            masks[i, g, y:y + h, x:x + w] = 1
            boxes[i, g] = (y, x, y + h, x + w)
        for j in range(S):
            g = rs.randint(0, N_GT[i])
            assign[i * S + j] = g
            b = boxes[i, g]
            roi[i * S + j] = b + rs.uniform(-0.15, 0.15, 4) * np.tile(b[2:] - b[:2], 2)
    Rm = N * ROWS
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    masks_d, roi_d, assign_d = t(masks), t(roi), t(assign)
    n_gt, n_pos = t(np.asarray(N_GT, np.int32)), t(np.full((N,), ROWS, np.int32))
    label = t(rs.randint(1, N_FG + 1, Rm).astype(np.int32))
    mask_out = torch.randn((Rm, 28, 28, CP), device=dev)
    gt28 = t(rs.randint(0, 2, (Rm, 28, 28)).astype(np.int32))
    feat = torch.randn((Rm, 14, 14, C), device=dev)
    cin_p = C + 32
    g_in, g_pool = torch.randn((Rm, 14, 14, cin_p), device=dev), torch.randn((Rm, 14, 14, C), device=dev)
    pred, tgt = torch.randn((Rm, CP), device=dev), torch.rand((Rm,), device=dev)
    D = 100
    score, dlab, dpred = torch.rand((D,), device=dev), t(rs.randint(0, N_FG, D).astype(np.int32)), torch.randn((D, CP), device=dev)
    area = sum(int((boxes[i, g, 2] - boxes[i, g, 0]) * (boxes[i, g, 3] - boxes[i, g, 1])) for i in range(N) for g in range(N_GT[i]))
    crop = 0
    for r in range(Rm):
        b = roi[(r // ROWS) * S + r % ROWS]
        crop += max(min(int(b[2]), H) - max(int(b[0]), 0), 0) * max(min(int(b[3]), W) - max(int(b[1]), 0), 0)
    cases = [
        ('maskiou_target (2 launches)', sum(N_GT) * H * W + crop + Rm * 784 * (4 + 4) + Rm * 4,
         lambda i: ops.maskiou_target(masks_d, n_gt, roi_d, assign_d, label, n_pos, S, ROWS, mask_out, gt28, N_FG)),
        ('maskiou_input_fwd', Rm * 196 * (C + cin_p) * 4 + Rm * 784 * 4, lambda i: ops.maskiou_input_fwd(feat, mask_out, label, N_FG, cin_p)),
        ('maskiou_input_bwd', Rm * 196 * C * 4 * 3, lambda i: ops.maskiou_input_bwd(g_in, g_pool)),
        ('maskiou_l2 (3 launches)', Rm * (4 + 4 + 4) + Rm * CP * 4, lambda i: ops.maskiou_l2(pred, tgt, label, N_FG)),
        ('maskiou_rescore (D = %d)' % D, D * 16, lambda i: ops.maskiou_rescore(score, dpred, dlab, N_FG)),
    ]
    us = {name: [] for name, _, _ in cases}
    for _, _, fn in cases:
        _event_ms(fn, 5)
    for _ in range(args.reps):
        for name, _, fn in cases:
            us[name].append(_event_ms(fn, 20) * 1e3)
    return {'shape': {'batch': N, 'size': args.size, 'mask_slots': G, 'n_gt': list(N_GT), 'mask_rows': Rm, 'channels': C, 'classes': N_FG,
                      'mask_bytes_counted': sum(N_GT) * H * W, 'mask_area_px': area},
            'kernels': [{'call': name, 'us_median': round(statistics.median(us[name]), 2), 'us_min': round(min(us[name]), 2),
                         'us_max': round(max(us[name]), 2), 'min_bytes': int(nbytes),
                         'GBps_at_median': round(nbytes / statistics.median(us[name]) / 1e3, 1),
                         'note': 'through the Python wrapper: output allocation and the ctypes call are in the window'}
                        for name, nbytes, _ in cases]}


def step_table(args, dev):
    import torch
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import DEFAULT_GEMM_ARITHMETIC, FPNMaskRCNNTrainChain, calc_mask_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay
    from chainer_maskrcnn.utils.synthetic import make_batch
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    variants = {}
    for name, on in (('off', False), ('on', True)):
        model = MaskRCNN(n_fg_class=80, device=dev, mask_iou=on)
        chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic=DEFAULT_GEMM_ARITHMETIC)
        opt = MomentumSGD(lr=1e-4).setup(chain)
        opt.add_hook(WeightDecay(5e-4))
        if variants:                    # one set of streams for both trainers (tools/cascade_bench.py)
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
    rows = [{'mask_iou': name, 'step_ms_median': round(statistics.median(ms[name]), 3), 'step_ms_min': round(min(ms[name]), 3),
             'step_ms_max': round(max(ms[name]), 3), 'step_ms_all': [round(v, 3) for v in ms[name]],
             'vs_off': round(statistics.median(ms[name]) / base, 4), 'images_per_s': round(2000.0 / statistics.median(ms[name]), 2),
             'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1), 'losses_finite': finite[name],
             'n_params': variants[name][1].faster_rcnn.ps.n_params()} for name in variants]
    rows[1]['peak_delta_MiB'] = round((peak['on'] - peak['off']) / 2 ** 20, 1)
    rows[1]['maskiou_loss'] = float(variants['on'][1].observation['maskiou_loss'])
    rows[1]['note'] = 'both models are resident in both windows: the peak is that of the process, its delta that of the MaskIoU step'
    return {'step': rows}


def run_part(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('maskiou_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(dev)}
    res.update(kernel_table(args, dev) if args.part == 'kernels' else step_table(args, dev))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', default='all', choices=['all', 'kernels', 'step'], help='all: each part in a child process with its own time limit')
    ap.add_argument('--steps', type=int, default=10, help='steps per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if args.part != 'all':
        return run_part(args)
    res = {'size': args.size, 'batch': 2}
    for part in ('kernels', 'step'):        # a fresh process per part; a part that fails or runs out of time ends the run: nothing starts after it
        cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--steps', str(args.steps), '--reps', str(args.reps), '--size', str(args.size)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=LIMITS[part], check=False)
        except subprocess.TimeoutExpired:
            raise SystemExit('maskiou_bench.py: part %r did not finish within %d s' % (part, LIMITS[part]))
        if p.returncode != 0:
            raise SystemExit('maskiou_bench.py: part %r ended with status %d' % (part, p.returncode))
        res.update(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
