#!/usr/bin/env python3
"""What GroupNorm in the FPN costs on the device.  Two parts, each a child process under its own time limit; the parent
never opens the device and stops at the first part that fails.
  kernels   device time (HIP events, median of --reps windows of 20 calls) of mrcnn_group_norm_map_fwd_f32 / _bwd_f32 at the four maps the
            FPN normalises at batch size 2 and 1024 x 1024 - (2,256,256,256), (2,128,128,256), (2,64,64,256), (2,32,32,256), 32 groups -
            beside the minimum bytes of the call (forward 2 |x|: x in, y out; backward 3 |x|: gy, x in, gx out), the bytes the design moves
            (forward 3 |x|: x twice; backward 5 |x|: gy and x twice), both over the time as a fraction of 8 TB/s, and beside the existing
            generic entry point mrcnn_group_norm_fwd_f32 / _bwd_f32 on the same tensors.  Every call works on its own set of tensors out of
            a ring larger than the 256 MiB last-level cache, so the bytes come from HBM.
  step      the bs-2 1024 x 1024 mask training step with fpn_norm off (the step without this feature) and on, two models in one process,
            windows alternating: step time (device events, median), peak allocated memory of a window and its delta.  The two trainers
            share their auxiliary and step streams (tools/groupnorm_bench.py found a second pair of streams to cost 16 ms a step).
Prints one JSON object.

usage: fpn_groupnorm_bench.py [--steps 10] [--reps 5] [--size 1024] [--skip-step 0] [--commit TEXT] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)

HBM_PEAK = 8e12                    # bytes/s, MI355X
SHAPES = [(2, 256, 256, 256), (2, 128, 128, 256), (2, 64, 64, 256), (2, 32, 32, 256)]
GROUPS = 32
RING_BYTES = 1 << 30
PART_LIMIT_S = {'kernels': 240, 'step': 420}


def _event_ms(torch, fn, n):
    """Milliseconds per call of fn over n back-to-back calls, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_table(args, torch, dev):
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    lib, ptr, sp = _hip.lib(), _hip.ptr, _hip.stream_ptr
    rows = []
    for shape in SHAPES:
        Rn, H, W, C = shape
        G = GROUPS
        nx = Rn * H * W * C * 4
        ring = max(2, int(math.ceil(RING_BYTES / (3.0 * nx))))
        xs = [torch.randn(shape, device=dev) * 2 + 3 for _ in range(ring)]
        gys = [torch.randn(shape, device=dev) for _ in range(ring)]
        outs = [torch.empty(shape, device=dev) for _ in range(ring)]
        gamma, beta = torch.randn(C, device=dev) * 0.1 + 1, torch.randn(C, device=dev) * 0.1
        gg, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
        mean, rstd = torch.empty((Rn, G), device=dev), torch.empty((Rn, G), device=dev)
        ppc, chunks, nf, nb = ops.group_norm_map_plan(Rn, H, W, C, C, G)
        path, nb_gen = ops.group_norm_plan(Rn, H, W, C, C, G)
        ws = torch.empty((max(nf, nb, nb_gen, 16),), dtype=torch.uint8, device=dev)

        def map_fwd(i):
            k = i % ring
            _hip.check(lib.mrcnn_group_norm_map_fwd_f32(ptr(xs[k]), ptr(gamma), ptr(beta), Rn, H, W, C, C, G, 1e-5, ptr(outs[k]), ptr(mean), ptr(rstd),
                                                        ptr(ws), ws.numel(), sp()))

        def map_bwd(i):
            k = i % ring
            _hip.check(lib.mrcnn_group_norm_map_bwd_f32(ptr(gys[k]), ptr(xs[k]), ptr(gamma), ptr(mean), ptr(rstd), Rn, H, W, C, C, G, ptr(outs[k]),
                                                        ptr(gg), ptr(gb), 0, ptr(ws), ws.numel(), sp()))

        def gen_fwd(i):
            k = i % ring
            _hip.check(lib.mrcnn_group_norm_fwd_f32(ptr(xs[k]), ptr(gamma), ptr(beta), Rn, H, W, C, C, G, 1e-5, 0, ptr(outs[k]), ptr(mean), ptr(rstd),
                                                    sp()))

        def gen_bwd(i):
            k = i % ring
            _hip.check(lib.mrcnn_group_norm_bwd_f32(ptr(gys[k]), ptr(xs[k]), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), Rn, H, W, C, C, G, 0,
                                                    ptr(outs[k]), ptr(gg), ptr(gb), 0, ptr(ws), ws.numel(), sp()))
        map_fwd(0)                          # the statistics of set 0 serve every backward call: the time does not depend on their values
        cases = [('map', 'forward', 2 * nx, 3 * nx, map_fwd), ('map', 'backward', 3 * nx, 5 * nx, map_bwd),
                 (ops.GN_PATHS[path], 'forward', 2 * nx, None, gen_fwd), (ops.GN_PATHS[path], 'backward', 3 * nx, None, gen_bwd)]
        us = {c[:2]: [] for c in cases}
        for c in cases:
            _event_ms(torch, c[4], 5)
        for _ in range(args.reps):
            for c in cases:
                us[c[:2]].append(_event_ms(torch, c[4], 20) * 1e3)
        for kernels, call, min_bytes, moved, _ in cases:
            t = statistics.median(us[(kernels, call)])
            row = {'shape': list(shape), 'groups': G, 'kernels': kernels, 'call': call, 'us_median': round(t, 2),
                   'us_all': [round(v, 2) for v in us[(kernels, call)]], 'min_bytes': int(min_bytes),
                   'fraction_of_8TBps_min_bytes': round(min_bytes / (t * 1e-6) / HBM_PEAK, 3), 'ring_sets': ring}
            if kernels == 'map':
                row.update({'design_bytes': int(moved), 'fraction_of_8TBps_design_bytes': round(moved / (t * 1e-6) / HBM_PEAK, 3),
                            'pixels_per_chunk': ppc, 'workgroups': Rn * chunks,
                            'speedup_over_generic': None})
            rows.append(row)
        for call in ('forward', 'backward'):
            m = [r for r in rows if r['shape'] == list(shape) and r['call'] == call]
            m[0]['speedup_over_generic'] = round(m[1]['us_median'] / m[0]['us_median'], 2)
        del xs, gys, outs
        torch.cuda.empty_cache()
    return rows


def step_table(args, torch, dev):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay
    from chainer_maskrcnn.utils.synthetic import make_batch
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    variants = {}
    for name, norm in (('none', None), ('gn', 'gn')):
        model = MaskRCNN(n_fg_class=80, device=dev, fpn_norm=norm)
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
            ms[name].append(_event_ms(torch, lambda i: opt.update(chain, *batch, 1.0), args.steps))
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated(dev))
            finite[name] = bool(torch.isfinite(chain.observation['loss']).item())
    base = statistics.median(ms['none'])
    rows = [{'fpn_norm': name, 'step_ms_median': round(statistics.median(ms[name]), 3), 'step_ms_all': [round(v, 3) for v in ms[name]],
             'vs_none': round(statistics.median(ms[name]) / base, 4), 'images_per_s': round(2000.0 / statistics.median(ms[name]), 2),
             'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1), 'loss_finite': finite[name],
             'n_params': variants[name][1].faster_rcnn.ps.n_params()} for name in variants]
    rows[1]['step_delta_ms'] = round(statistics.median(ms['gn']) - base, 3)
    rows[1]['peak_delta_MiB'] = round((peak['gn'] - peak['none']) / 2 ** 20, 1)
    rows[1]['note'] = 'both models are resident in both windows: the peak is that of the process, its delta that of the GroupNorm step'
    rows[1]['streams_shared'] = all(c._aux is variants['none'][1]._aux and o._hi is variants['none'][0]._hi for o, c in variants.values())
    return rows


def run_part(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fpn_groupnorm_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(dev)}
    res[args.part] = kernel_table(args, torch, dev) if args.part == 'kernels' else step_table(args, torch, dev)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10, help='steps per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--skip-step', type=int, default=0, choices=[0, 1], help='1: the kernel table only')
    ap.add_argument('--commit', default='', help='recorded in the result: the commit the numbers were taken on')
    ap.add_argument('--out', default='')
    ap.add_argument('--part', default='', choices=['', 'kernels', 'step'], help='(internal) run one part in this process')
    args = ap.parse_args()
    if args.part:
        return run_part(args)
    res = {'size': args.size, 'batch': 2, 'commit': args.commit,
           'expected': {'normalised_maps_MB': 354, 'kernel_bytes_per_step_GB': 2.8, 'peak_delta_MiB': 354,
                        'note': 'expectations from the bytes (eight maps, forward 3 |x| + backward 5 |x|), not bars'}}
    tmp = tempfile.mkdtemp(prefix='fpn_gn_bench_')
    for part in ('kernels',) + (() if args.skip_step else ('step',)):
        out = os.path.join(tmp, part + '.json')
        cmd = ['timeout', '-k', '10', str(PART_LIMIT_S[part]), sys.executable, os.path.abspath(__file__), '--part', part, '--out', out,
               '--steps', str(args.steps), '--reps', str(args.reps), '--size', str(args.size)]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit('fpn_groupnorm_bench.py: part %r ended with status %d; nothing after it was started' % (part, rc))
        with open(out) as f:
            res.update(json.load(f))
    slower = [r for r in res['kernels'] if r['kernels'] == 'map' and not r['speedup_over_generic'] > 1.0]
    res['map_faster_than_generic_at_every_shape'] = not slower
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
