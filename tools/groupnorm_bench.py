#!/usr/bin/env python3
"""What GroupNorm in the RoI heads costs on the device, measured in ONE process with the variants interleaved:
  kernels   device time (HIP events, median of --reps windows of 20 calls) of mrcnn_group_norm_fwd_f32 / _bwd_f32 at the head's shapes
            (512,7,7,256), (256,14,14,256), (512,14,14,256), 32 groups, beside the minimum bytes of the call - forward 2 |x| (x in, y
            out), backward 3 |x| (gy, x in, gx out) + the partial rows (written and read once) - and that minimum over the time as a
            fraction of 8 TB/s.  Every call works on its own set of tensors out of a ring larger than the 256 MB Infinity Cache, so the
            bytes come from HBM.  The path is decided by the geometry alone (mrcnn_group_norm_plan): with 32 groups these shapes take the
            register-resident kernels; the generic kernels are timed on the same tensors with the nearest grouping that takes them (4 groups
            at 14 x 14, 1 group at 7 x 7), labelled as such.
  step      the bs-2 1024 x 1024 mask training step with --head-norm none and gn, two models in one process, windows alternating: step
            time (device events, median), peak allocated memory of a window and its delta.  The two trainers share their auxiliary and
            step streams: with a pair of streams of its own the trainer built second runs at 37 instead of 21 ms per step whatever its
            architecture (two plain models measured 21.3 and 37.4 ms) - supposedly its streams no longer fit the 4 hardware queues a
            process opens by default.
Prints one JSON object.

usage: groupnorm_bench.py [--steps 10] [--reps 5] [--size 1024] [--skip-step 0] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)
import torch  # noqa: E402

HBM_PEAK = 8e12                    # bytes/s, MI355X
SHAPES = [(512, 7, 7, 256), (256, 14, 14, 256), (512, 14, 14, 256)]
RING_BYTES = 1 << 30


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
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    lib, ptr, sp = _hip.lib(), _hip.ptr, _hip.stream_ptr
    rows = []
    for shape in SHAPES:
        Rn, H, W, C = shape
        nx = Rn * H * W * C * 4
        variants = [(32, 'the head\'s 32 groups')]
        for G in (16, 8, 4, 2, 1):         # the nearest grouping the plan routes to the generic kernels
            if ops.group_norm_plan(Rn, H, W, C, C, G)[0] == 1:
                variants.append((G, 'generic kernels: the same tensors in %d group(s)' % G))
                break
        ring = max(2, int(math.ceil(RING_BYTES / (3.0 * nx))))
        g = torch.Generator(device='cpu').manual_seed(Rn + H)
        xs = [(torch.randn(shape, generator=g) * 2 + 3).to(dev) for _ in range(ring)]
        gys = [torch.randn(shape, generator=g).to(dev) for _ in range(ring)]
        outs = [torch.empty(shape, device=dev) for _ in range(ring)]
        gamma, beta = (torch.randn(C, generator=g) * 0.1 + 1).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
        gg, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
        for G, label in variants:
            path, ws_bytes = ops.group_norm_plan(Rn, H, W, C, C, G)
            mean, rstd = torch.empty((Rn, G), device=dev), torch.empty((Rn, G), device=dev)
            ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)

            def fwd(i):
                k = i % ring
                _hip.check(lib.mrcnn_group_norm_fwd_f32(ptr(xs[k]), ptr(gamma), ptr(beta), Rn, H, W, C, C, G, 1e-5, 1, ptr(outs[k]), ptr(mean),
                                                        ptr(rstd), sp()))

            def bwd(i):
                k = i % ring
                _hip.check(lib.mrcnn_group_norm_bwd_f32(ptr(gys[k]), ptr(xs[k]), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), Rn, H, W, C, C, G, 0,
                                                        ptr(outs[k]), ptr(gg), ptr(gb), 0, ptr(ws), ws.numel(), sp()))
            fwd(0)                          # the statistics of set 0 serve every backward call: the time does not depend on their values
            cases = [('forward', 2 * nx, fwd), ('backward', 3 * nx + 2 * ws_bytes, bwd)]
            us = {name: [] for name, _, _ in cases}
            for name, _, fn in cases:
                _event_ms(fn, 5)
            for _ in range(args.reps):
                for name, _, fn in cases:
                    us[name].append(_event_ms(fn, 20) * 1e3)
            for name, nbytes, _ in cases:
                t = statistics.median(us[name])
                rows.append({'shape': list(shape), 'groups': G, 'path': ops.GN_PATHS[path], 'what': label, 'call': name,
                             'us_median': round(t, 2), 'us_all': [round(v, 2) for v in us[name]], 'min_bytes': int(nbytes),
                             'TB_per_s_of_min_bytes': round(nbytes / (t * 1e-6) / 1e12, 3),
                             'fraction_of_8TBps': round(nbytes / (t * 1e-6) / HBM_PEAK, 3), 'ring_sets': ring})
        del xs, gys, outs
        torch.cuda.empty_cache()
    return rows


def step_table(args, dev):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay
    from chainer_maskrcnn.utils.synthetic import make_batch
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    variants = {}
    for name, norm in (('none', None), ('gn', 'gn')):
        model = MaskRCNN(n_fg_class=80, device=dev, head_norm=norm)
        chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic='bf16x6_behind_backbone')
        opt = MomentumSGD(lr=1e-4).setup(chain)
        opt.add_hook(WeightDecay(5e-4))
        if variants:                    # one set of streams for both trainers (see the module text)
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
            finite[name] = bool(torch.isfinite(chain.observation['loss']).item())
    base = statistics.median(ms['none'])
    rows = [{'head_norm': name, 'step_ms_median': round(statistics.median(ms[name]), 3), 'step_ms_all': [round(v, 3) for v in ms[name]],
             'vs_none': round(statistics.median(ms[name]) / base, 4), 'images_per_s': round(2000.0 / statistics.median(ms[name]), 2),
             'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1), 'loss_finite': finite[name],
             'n_params': variants[name][1].faster_rcnn.ps.n_params()} for name in variants]
    rows[1]['peak_delta_MiB'] = round((peak['gn'] - peak['none']) / 2 ** 20, 1)
    rows[1]['note'] = 'both models are resident in both windows: the peak is that of the process, its delta that of the GroupNorm step'
    rows[1]['streams_shared'] = all(c._aux is variants['none'][1]._aux and o._hi is variants['none'][0]._hi for o, c in variants.values())
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
        raise SystemExit('groupnorm_bench.py measures on a HIP device; none found')
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
