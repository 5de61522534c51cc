"""What freezing costs and buys on the device, measured in ONE process with the variants interleaved (boxes and runs differ by a few
per cent): the bs-2 1024x1024 training step with freezing off, with freeze_bn, and with freeze_bn + freeze_at 2 - step
time (device events, median), peak allocated memory - and the standalone rate of the frozen-BatchNorm kernels (csrc/bn_frozen.hip) at
the res2 and res4 shapes of that step beside k_bn_infer's on the same tensors.  Prints one JSON object.

usage: freeze_bench.py [--steps 10] [--reps 5] [--size 1024] [--out FILE]
A rate here is algorithmic bytes (each tensor once) over kernel time; it is not a share of any peak."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)
import torch  # noqa: E402

VARIANTS = [('off', (False, 0)), ('freeze_bn', (True, 0)), ('freeze_bn+freeze_at_2', (True, 2))]


def _event_ms(fn, n):
    """Milliseconds per call of fn over n back-to-back calls, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def step_table(args, dev):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay
    from chainer_maskrcnn.utils.synthetic import make_batch
    model = MaskRCNN(n_fg_class=80, device=dev)
    chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic='bf16x6_behind_backbone')
    opt = MomentumSGD(lr=1e-4).setup(chain)
    opt.add_hook(WeightDecay(5e-4))
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    # running statistics that fit the data (the frozen layers use them; fresh (0, 1) buffers make the activations explode): 30 training-mode
    # steps, which also warm the unfrozen variant up
    for _ in range(30):
        opt.update(chain, *batch, 1.0)
    for _, fz in VARIANTS[1:]:
        model.freeze(*fz)
        for _ in range(3):
            opt.update(chain, *batch, 1.0)
    ms = {name: [] for name, _ in VARIANTS}
    peak = {name: 0 for name, _ in VARIANTS}
    finite = {}
    for _ in range(args.reps):
        for name, fz in VARIANTS:
            model.freeze(*fz)
            opt.update(chain, *batch, 1.0)          # the variant's first step after the switch is not timed
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ms[name].append(_event_ms(lambda: opt.update(chain, *batch, 1.0), args.steps))
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated(dev))
            finite[name] = bool(torch.isfinite(chain.observation['loss']).item())
    model.freeze(False, 0)
    base = statistics.median(ms['off'])
    return [{'variant': name, 'step_ms_median': round(statistics.median(ms[name]), 3), 'step_ms_all': [round(v, 3) for v in ms[name]],
             'vs_off': round(statistics.median(ms[name]) / base, 4), 'images_per_s': round(2000.0 / statistics.median(ms[name]), 2),
             'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1), 'loss_finite': finite[name]} for name, _ in VARIANTS]


def kernel_table(args, dev):
    from chainer_maskrcnn._hip import ops
    s = args.size
    shapes = [('res2', 2 * (s // 4) * (s // 4), 256), ('res4', 2 * (s // 16) * (s // 16), 1024)]
    rows = []
    for stage, P, C in shapes:
        g = torch.Generator(device='cpu').manual_seed(P + C)
        mk = lambda *sh: torch.randn(*sh, generator=g).to(dev)
        xa, xb, gy = mk(P, C), mk(P, C), mk(P, C)
        ga, ba, ma, va = mk(C) * 0.1 + 1, mk(C) * 0.1, mk(C) * 0.1, torch.rand(C, generator=g).to(dev) + 0.5
        gb, bb, mb, vb = mk(C) * 0.1 + 1, mk(C) * 0.1, mk(C) * 0.1, torch.rand(C, generator=g).to(dev) + 0.5
        y = ops.bn_infer_fwd(xa, ga, ba, ma, va, xb, True)
        out, out2 = torch.empty_like(xa), torch.empty_like(xa)
        from chainer_maskrcnn import _hip
        lib, ptr, sp = _hip.lib(), _hip.ptr, _hip.stream_ptr

        def infer(res):         # k_bn_infer into a preallocated output (the yardstick: the same kind of streams)
            return lambda: _hip.check(lib.mrcnn_bn_infer_fwd_f32(ptr(xa), ptr(ga), ptr(ba), ptr(ma), ptr(va), ptr(res), ptr(out), P, C, 2e-5, 1, sp()))

        def bwd(mode, yx):
            return lambda: _hip.check(lib.mrcnn_bn_frozen_bwd_f32(ptr(gy), ptr(yx), ptr(ga), ptr(ba), ptr(ma), ptr(va), ptr(out), None, P, C, 2e-5, mode, sp()))
        cases = [('k_bn_infer (x -> y)', 8, infer(None)), ('k_bn_infer (x, residual -> y)', 12, infer(xb)),
                 ('bn_frozen_bwd mode 0', 8, bwd(0, None)), ('bn_frozen_bwd mode 1 (y)', 12, bwd(1, y)), ('bn_frozen_bwd mode 2 (x)', 12, bwd(2, xa)),
                 ('bn_infer_fwd_pair', 12, lambda: _hip.check(lib.mrcnn_bn_infer_fwd_pair_f32(ptr(xa), ptr(ga), ptr(ba), ptr(ma), ptr(va), ptr(xb), ptr(gb), ptr(bb),
                                                                                            ptr(mb), ptr(vb), ptr(out), P, C, 2e-5, sp()))),
                 ('bn_frozen_bwd_pair (y)', 16, lambda: _hip.check(lib.mrcnn_bn_frozen_bwd_pair_f32(ptr(gy), ptr(y), ptr(ga), ptr(va), ptr(gb), ptr(vb), ptr(out),
                                                                                                  ptr(out2), P, C, 2e-5, sp()))),
                 ('bn_frozen_bwd_pair (masked gy)', 12, lambda: _hip.check(lib.mrcnn_bn_frozen_bwd_pair_f32(ptr(gy), None, ptr(ga), ptr(va), ptr(gb), ptr(vb),
                                                                                                          ptr(out), ptr(out2), P, C, 2e-5, sp())))]
        us = {name: [] for name, _, _ in cases}
        for name, _, fn in cases:
            _event_ms(fn, 5)
        for _ in range(args.reps):
            for name, _, fn in cases:
                us[name].append(_event_ms(fn, 20) * 1e3)
        ref = {8: None, 12: None}
        for name, bpe, _ in cases:
            t = statistics.median(us[name])
            gbs = bpe * P * C / (t * 1e-6) / 1e9
            if name.startswith('k_bn_infer'):
                ref[bpe] = gbs
            rows.append({'shape': '%s (P=%d, C=%d, %.0f MB per tensor)' % (stage, P, C, P * C * 4 / 1e6), 'kernel': name, 'bytes_per_element': bpe,
                         'us_median': round(t, 2), 'GB_per_s': round(gbs, 1),
                         'of_k_bn_infer': None if name.startswith('k_bn_infer') else round(gbs / ref[12 if bpe >= 12 else 8], 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10, help='steps per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('freeze_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(dev), 'size': args.size, 'batch': 2, 'kernels': kernel_table(args, dev),
           'step': step_table(args, dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
