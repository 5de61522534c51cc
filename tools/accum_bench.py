"""What gradient accumulation and gradient clipping cost on the device, measured in ONE process with the variants interleaved (boxes and
runs differ by a few per cent): the bs-2 1024x1024 training step (a) plain, (b) as the micro-batches of --accum-steps 4
(3 x accumulate + 1 update; the time is per micro-batch), (c) plain with --grad-clip - device-event medians, peak allocated memory - and
the standalone rate of the three kernels of csrc/optim.hip over the model's flat buffers beside k_sgd's.  Prints one JSON object.

usage: accum_bench.py [--steps 8] [--reps 5] [--size 1024] [--accum-steps 4] [--grad-clip 10] [--out FILE]
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
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay, GradientClipping
    from chainer_maskrcnn.utils.synthetic import make_batch
    model = MaskRCNN(n_fg_class=80, device=dev)
    chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, mask_rows='all', gemm_arithmetic='bf16x6_behind_backbone')
    # one model, two optimizers over its buffers: the plain one and the clipping one (lr 0: the timed variants all see the same weights)
    opt = MomentumSGD(lr=0.0).setup(chain)
    opt.add_hook(WeightDecay(5e-4))
    clip = MomentumSGD(lr=0.0).setup(chain)
    clip.add_hook(WeightDecay(5e-4))
    clip.add_hook(GradientClipping(args.grad_clip))
    b = make_batch(100, 2, args.size, args.size, G=8)
    batch = [torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'masks')]
    K = args.accum_steps

    def plain():
        opt.update(chain, *batch, 1.0)

    def accumulated():          # one update of K micro-batches
        for _ in range(K - 1):
            opt.accumulate(chain, *batch, 1.0)
        opt.update(chain, *batch, 1.0)

    def clipped():
        clip.update(chain, *batch, 1.0)
    variants = [('plain', plain, 1), ('accum_steps_%d' % K, accumulated, K), ('grad_clip', clipped, 1)]
    for _ in range(5):
        plain()
    for _, fn, _ in variants[1:]:
        fn()
    ms = {name: [] for name, _, _ in variants}
    peak = {name: 0 for name, _, _ in variants}
    for _ in range(args.reps):
        for name, fn, micro in variants:
            fn()                                    # the variant's first step after the switch is not timed
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ms[name].append(_event_ms(fn, max(1, args.steps // micro)) / micro)
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated(dev))
    base = statistics.median(ms['plain'])
    spread = max(ms['plain']) - min(ms['plain'])
    rows = []
    for name, _, _ in variants:
        med = statistics.median(ms[name])
        rows.append({'variant': name, 'micro_batch_ms_median': round(med, 3), 'micro_batch_ms_all': [round(v, 3) for v in ms[name]],
                     'minus_plain_ms': round(med - base, 3), 'within_plain_spread': bool(med - base <= spread),
                     'images_per_s': round(2000.0 / med, 2), 'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1)})
    return {'plain_spread_ms': round(spread, 3), 'grad_norm': float(clip.grad_norm), 'skipped_updates': int(clip.skipped_updates),
            'variants': rows}, model


def kernel_table(args, model):
    from chainer_maskrcnn._hip import ops
    ps = model.ps
    n = ps.params.numel()
    p, g, v, acc = ps.params.clone(), torch.randn_like(ps.grads) * 1e-3, torch.zeros_like(ps.momentum), torch.randn_like(ps.grads) * 1e-3
    hyper = torch.zeros(ops.HYPER_FLOATS, device=p.device)
    hyper[ops.HYPER_A], hyper[ops.HYPER_THRESHOLD], hyper[ops.HYPER_SCALE] = 1.0, 10.0, 1.0         # lr 0
    ws = ops.grad_norm_workspace(n, p.device)
    cases = [('k_sgd (the plain update)', 20, lambda: ops.sgd_momentum_wd(p, g, v, 0.0, 0.9, 5e-4)),
             ('k_accumulate first (acc = g)', 8, lambda: ops.grad_accumulate(acc, g, first=True)),
             ('k_accumulate (acc += g)', 12, lambda: ops.grad_accumulate(acc, g)),
             ('k_sqnorm + k_norm_finish (g)', 4, lambda: ops.grad_norm_hyper(g, hyper, ws=ws)),
             ('k_sqnorm + k_norm_finish (acc + g)', 8, lambda: ops.grad_norm_hyper(g, hyper, acc, ws=ws)),
             ('k_sgd_hyper (g)', 20, lambda: ops.sgd_momentum_wd_hyper(p, g, v, hyper)),
             ('k_sgd_hyper (acc + g)', 24, lambda: ops.sgd_momentum_wd_hyper(p, g, v, hyper, acc))]
    us = {name: [] for name, _, _ in cases}
    for _, _, fn in cases:
        _event_ms(fn, 5)
    for _ in range(args.reps):
        for name, _, fn in cases:
            us[name].append(_event_ms(fn, 20) * 1e3)
    rows = []
    for name, bpe, _ in cases:
        t = statistics.median(us[name])
        rows.append({'kernel': name, 'parameters': n, 'bytes_per_parameter': bpe, 'us_median': round(t, 2),
                     'GB_per_s': round(bpe * n / (t * 1e-6) / 1e9, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=8, help='micro-batches per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--accum-steps', type=int, default=4)
    ap.add_argument('--grad-clip', type=float, default=10.0)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('accum_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    step, model = step_table(args, dev)
    res = {'device': torch.cuda.get_device_name(dev), 'size': args.size, 'batch': 2, 'accum_steps': args.accum_steps,
           'grad_clip': args.grad_clip, 'step': step, 'kernels': kernel_table(args, model)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
