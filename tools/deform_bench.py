#!/usr/bin/env python3
"""What deformable convolution in res3-res5 costs on the device.  Three parts, each a child process under its own time
limit; the parent never opens the device and stops at the first part that fails.
  kernels   device time (HIP events, median of --reps windows of 10 calls) of mrcnn_deform_cols_fwd_f32, mrcnn_deform_offset_bwd_f32 and
            mrcnn_deform_input_bwd_f32 at the res3 / res4 / res5 shapes of a bs-2 1024 x 1024 step - (2,128,128,128), (2,64,64,256),
            (2,32,32,512) -, v1 and v2, beside the minimum bytes of the call (cols forward: x and the offsets in, 9 |x| out; offset gradient:
            9 |x| + |x| + the offsets in, their gradient out; input gradient: 9 |x| + the offsets in, |x| out), on trained-looking offsets
            (normal, sigma 1.5 cells) and on adversarial ones (every tap of every pixel aimed at one cell of its image), with the median and
            the maximum length of the destination lists of the input gradient.  Every call works on its own set of tensors - inputs AND
            outputs, through the C entry points on preallocated buffers - out of a ring larger than the 256 MiB last-level cache.
  step      the bs-2 1024 x 1024 mask training step with the feature off, with v1 and with v2 in all three stages: three models in one
            process, windows alternating; step time (device events, median) and the peak allocated memory of a window.  The trainers share
            their auxiliary and step streams.
  predict   MaskRCNN.predict of one 1024 x 1024 image with the feature off, v1 and v2 (the same seed: the shared parameters are equal, the
            offset convolutions zero), windows alternating; milliseconds per image (device events, median).
Prints one JSON object.

usage: deform_bench.py [--steps 10] [--reps 5] [--size 1024] [--parts kernels step predict] [--commit TEXT] [--out FILE]"""
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
STAGES = ('res3', 'res4', 'res5')
RING_BYTES = 1 << 30
PARTS = ('kernels', 'step', 'predict')
PART_LIMIT_S = {'kernels': 300, 'step': 420, 'predict': 240}
LD = 32
VARIANTS = (('off', None, False), ('v1', STAGES, False), ('v2', STAGES, True))


def _event_ms(torch, fn, n):
    """Milliseconds per call of fn over n back-to-back calls, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def stage_shapes(size):
    return [(s, (2, size // st, size // st, c)) for s, st, c in (('res3', 8, 128), ('res4', 16, 256), ('res5', 32, 512))]


def make_offsets(torch, kind, shape, dev, seed):
    N, H, W, _ = shape
    g = torch.Generator(device='cpu').manual_seed(seed)
    off = torch.zeros((N, H, W, LD))
    if kind == 'trained':
        off[..., :18] = 1.5 * torch.randn((N, H, W, 18), generator=g)
    else:                           # every tap of every pixel at the cell (H / 2, W / 2) of its image, a quarter of a cell inside it
        ys, xs = torch.arange(H).view(1, H, 1, 1).float(), torch.arange(W).view(1, 1, W, 1).float()
        ti, tj = (torch.arange(9) // 3).float().view(1, 1, 1, 9), (torch.arange(9) % 3).float().view(1, 1, 1, 9)
        off[..., 0:18:2] = (H // 2 + 0.25) - (ys - 1 + ti)
        off[..., 1:18:2] = (W // 2 + 0.25) - (xs - 1 + tj)
    off[..., 18:27] = torch.randn((N, H, W, 9), generator=g)
    return off.to(dev)


def list_lengths(torch, off, shape):
    """Entries per destination pixel of the input gradient's inverted index, by the rule of csrc/deform_common.h restated in torch."""
    N, H, W, _ = shape
    dev = off.device
    n_ = torch.arange(N, device=dev).view(N, 1, 1)
    ys, xs = torch.arange(H, device=dev).view(1, H, 1), torch.arange(W, device=dev).view(1, 1, W)
    counts = torch.zeros((N * H * W,), dtype=torch.int64, device=dev)
    for k in range(9):
        py = (ys - 1 + k // 3).float() + off[..., 2 * k]
        px = (xs - 1 + k % 3).float() + off[..., 2 * k + 1]
        inside = (py > -1) & (py < H) & (px > -1) & (px < W)
        y0, x0 = torch.floor(torch.where(inside, py, torch.zeros_like(py))).long(), torch.floor(torch.where(inside, px, torch.zeros_like(px))).long()
        for a in (0, 1):
            for b in (0, 1):
                yy, xx = y0 + a, x0 + b
                ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                idx = ((n_ * H + yy.clamp(0, H - 1)) * W + xx.clamp(0, W - 1))[ok]
                counts += torch.bincount(idx, minlength=N * H * W)
    return {'median': float(counts.float().median().item()), 'max': int(counts.max().item()), 'mean': round(float(counts.float().mean().item()), 2),
            'entries': int(counts.sum().item())}


def kernel_table(args, torch, dev):
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops
    lib, ptr, sp = _hip.lib(), _hip.ptr, _hip.stream_ptr
    rows = []
    for stage, shape in stage_shapes(args.size):
        N, H, W, C = shape
        nx, noff = N * H * W * C * 4, N * H * W * LD * 4
        ring = max(2, int(math.ceil(RING_BYTES / (20.0 * nx))))
        xs = [torch.randn(shape, device=dev) for _ in range(ring)]
        gcs = [torch.randn((N, H, W, 9 * C), device=dev) for _ in range(ring)]
        o_cols = [torch.empty((N, H, W, 9 * C), device=dev) for _ in range(ring)]
        o_off = [torch.empty((N, H, W, LD), device=dev) for _ in range(ring)]
        o_gx = [torch.empty(shape, device=dev) for _ in range(ring)]
        ws = torch.empty((lib.mrcnn_deform_input_bwd_workspace_bytes(N, H, W),), dtype=torch.uint8, device=dev)
        geom = (N, H, W, C) + ops.DEFORM_GEOMETRY
        for kind in ('trained', 'adversarial'):
            offs = [make_offsets(torch, kind, shape, dev, 5 + i) for i in range(ring)]
            lengths = list_lengths(torch, offs[0], shape)
            for modulated in (False, True):
                n_read = 4 * N * H * W * (27 if modulated else 18)
                m = int(modulated)

                def cols_fwd(i):
                    k = i % ring
                    _hip.check(lib.mrcnn_deform_cols_fwd_f32(ptr(xs[k]), ptr(offs[k]), LD, m, *geom, ptr(o_cols[k]), sp()))

                def offset_bwd(i):
                    k = i % ring
                    _hip.check(lib.mrcnn_deform_offset_bwd_f32(ptr(gcs[k]), ptr(xs[k]), ptr(offs[k]), LD, m, *geom, ptr(o_off[k]), sp()))

                def input_bwd(i):
                    k = i % ring
                    _hip.check(lib.mrcnn_deform_input_bwd_f32(ptr(gcs[k]), ptr(offs[k]), LD, m, *geom, ptr(o_gx[k]), None, 0, ptr(ws), ws.numel(), sp()))
                cases = [('cols_fwd', nx + n_read + 9 * nx, cols_fwd), ('offset_bwd', 9 * nx + nx + n_read + noff, offset_bwd),
                         ('input_bwd', 9 * nx + n_read + nx, input_bwd)]
                us = {c[0]: [] for c in cases}
                for c in cases:
                    _event_ms(torch, c[2], 3)
                for _ in range(args.reps):
                    for c in cases:
                        us[c[0]].append(_event_ms(torch, c[2], 10) * 1e3)
                for call, min_bytes, _ in cases:
                    t = statistics.median(us[call])
                    rows.append({'stage': stage, 'shape': list(shape), 'version': 'v2' if modulated else 'v1', 'offsets': kind, 'call': call,
                                 'us_median': round(t, 2), 'us_all': [round(v, 2) for v in us[call]], 'min_bytes': int(min_bytes),
                                 'fraction_of_8TBps_min_bytes': round(min_bytes / (t * 1e-6) / HBM_PEAK, 3), 'ring_sets': ring,
                                 'list_length': lengths if call == 'input_bwd' else None})
            del offs
        del xs, gcs, o_cols, o_off, o_gx, ws
        torch.cuda.empty_cache()
    return rows


def _models(torch, dev, **kw):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    return {name: MaskRCNN(n_fg_class=80, device=dev, **dict(kw, **({} if stages is None else {'dcn_stages': stages, 'dcn_modulated': mod})))
            for name, stages, mod in VARIANTS}


def step_table(args, torch, dev):
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay
    from chainer_maskrcnn.utils.synthetic import make_batch
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    variants = {}
    for name, model in _models(torch, dev).items():
        chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic='bf16x6_behind_backbone')
        opt = MomentumSGD(lr=1e-4).setup(chain)
        opt.add_hook(WeightDecay(5e-4))
        if variants:                    # one set of streams for all trainers
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
    base = statistics.median(ms['off'])
    rows = []
    for name in variants:
        t = statistics.median(ms[name])
        rows.append({'dcn': name, 'step_ms_median': round(t, 3), 'step_ms_all': [round(v, 3) for v in ms[name]], 'vs_off': round(t / base, 4),
                     'step_delta_ms': round(t - base, 3), 'images_per_s': round(2000.0 / t, 2), 'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1),
                     'peak_delta_MiB': round((peak[name] - peak['off']) / 2 ** 20, 1), 'loss_finite': finite[name],
                     'n_params': variants[name][1].faster_rcnn.ps.n_params()})
    rows[0]['note'] = 'all three models are resident in every window: the peak is that of the process, its delta that of the variant\'s step'
    return rows


def predict_table(args, torch, dev):
    import numpy as np
    models = _models(torch, dev, min_size=args.size, max_size=args.size)
    rs = np.random.RandomState(0)
    img = torch.from_numpy((rs.rand(3, args.size, args.size) * 255).astype(np.float32))
    for m in models.values():
        m.use_preset('evaluate')
        m.use_max_detections(100)
        for _ in range(3):
            m.predict([img])
    torch.cuda.synchronize()
    ms = {name: [] for name in models}
    dets = {}
    for _ in range(args.reps):
        for name, m in models.items():
            m.predict([img])
            ms[name].append(_event_ms(torch, lambda i: m.predict([img]), args.steps))
            dets[name] = int(m.predict([img])[1][0].shape[0])
    base = statistics.median(ms['off'])
    return [{'dcn': name, 'predict_ms_median': round(statistics.median(ms[name]), 3), 'predict_ms_all': [round(v, 3) for v in ms[name]],
             'predict_delta_ms': round(statistics.median(ms[name]) - base, 3), 'detections': dets[name]} for name in models]


def run_part(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('deform_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(dev)}
    res[args.part] = {'kernels': kernel_table, 'step': step_table, 'predict': predict_table}[args.part](args, torch, dev)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10, help='steps (images) per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--parts', nargs='+', default=list(PARTS), choices=PARTS)
    ap.add_argument('--commit', default='', help='recorded in the result: the commit the numbers were taken on')
    ap.add_argument('--out', default='')
    ap.add_argument('--part', default='', choices=('',) + PARTS, help='(internal) run one part in this process')
    args = ap.parse_args()
    if args.part:
        return run_part(args)
    res = {'size': args.size, 'batch': 2, 'commit': args.commit,
           'note': 'no accuracy effect of the feature has been measured; cols (9 |x| per deformable layer) stay on the tape'}
    tmp = tempfile.mkdtemp(prefix='deform_bench_')
    for part in [p for p in PARTS if p in args.parts]:
        out = os.path.join(tmp, part + '.json')
        cmd = ['timeout', '-k', '10', str(PART_LIMIT_S[part]), sys.executable, os.path.abspath(__file__), '--part', part, '--out', out,
               '--steps', str(args.steps), '--reps', str(args.reps), '--size', str(args.size)]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit('deform_bench.py: part %r ended with status %d; nothing after it was started' % (part, rc))
        with open(out) as f:
            res.update(json.load(f))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
