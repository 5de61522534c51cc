#!/usr/bin/env python3
"""What PointRend costs on the device.  Three parts, each a child process of its own with its own time limit:
  kernels   device time (HIP events, median of --reps windows of 20 calls) of every new call at the workload's shape - batch 2, 1024 x 1024
            images (a 256 x 256 stride-4 level), the pos_cap = 64 mask rows per image, 196 points, 256 channels, 80 classes, and the two
            subdivision steps of D = 100 detections - beside the bytes a call must move at the least.
  step      the bs-2 1024 x 1024 mask training step of bench.py with point_rend off (the parent commit's step) and on, two trainers in one
            process, windows alternating: step time (device events, median and range of the windows), peak allocated memory and its delta.
  predict   the mask inference of D = 100 detections on one 1024 x 1024 pyramid - mask branch + paste - with the refinement off and on,
            windows alternating, per image.
Prints one JSON object; --out also writes it to a file.

usage: pointrend_bench.py [--part all|kernels|step|predict] [--steps 10] [--reps 5] [--size 1024] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)

N, G, S, ROWS, C, N_FG, CP, P, K, N_IMP, S0, HID, D = 2, 8, 256, 64, 256, 80, 96, 196, 3, 147, 28, 256, 100
LIMITS = {'kernels': 240, 'step': 480, 'predict': 300}          # seconds per part


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


def _boxes(rs, n, size):
    import numpy as np
    wh = rs.uniform(size / 16.0, size / 2.0, (n, 2))
    xy = rs.uniform(0, 1, (n, 2)) * (size - wh)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def kernel_table(args, dev):
    import numpy as np
    import torch
    from chainer_maskrcnn._hip import ops
    H = W = args.size
    rs = np.random.RandomState(1)
    Rm = N * ROWS
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rois = np.zeros((Rm, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), ROWS)
    rois[:, 1:] = _boxes(rs, Rm, args.size)
    rois_d = t(rois)
    masks = t((rs.rand(N, G, H, W) < 0.5).astype(np.uint8))
    n_gt, n_pos = t(np.full((N,), G, np.int32)), t(np.full((N,), ROWS, np.int32))
    assign = t(rs.randint(0, G, N * S).astype(np.int32))
    label = t(rs.randint(1, N_FG + 1, Rm).astype(np.int32))
    coarse = torch.randn((Rm, S0, S0, CP), device=dev)
    fmap = torch.randn((N, H // 4, W // 4, C), device=dev)
    g_map = torch.randn((N, H // 4, W // 4, C), device=dev)
    cin_p = (C + N_FG + 31) // 32 * 32
    n_keys = ops.point_n_keys(P, K * P, N_IMP)
    keys = t(rs.randint(0, 2 ** 32, (Rm, n_keys), dtype=np.uint64).astype(np.uint32).view(np.int32))
    coords = ops.point_train_coords(keys, coarse, label, N_FG, P, K * P, N_IMP)
    x_in = ops.point_features_fwd(coords, rois_d, fmap, 0.25, coarse, N_FG, cin_p)
    g_in = torch.randn_like(x_in)
    hid = torch.randn((Rm, 1, P, HID), device=dev)
    pred = torch.randn((Rm, 1, P, CP), device=dev)
    tgt = ops.point_target(masks, n_gt, rois_d, assign, label, n_pos, S, ROWS, coords)
    dlab = t(rs.randint(0, N_FG, D).astype(np.int32))
    dm = torch.randn((D, S0, S0, CP), device=dev)
    up1, idx1, _ = ops.point_subdivide(dm, dlab, N_FG, 784)
    g56 = up1.view(D, 56, 56, 1)
    up2, idx2, _ = ops.point_subdivide(g56, None, 1, 784)
    dpred = torch.randn((D, 1, 784, CP), device=dev)
    n_pt = Rm * P
    cases = [
        ('point_train_coords', Rm * (n_keys * 4 + K * P * 16 + P * 8), lambda i: ops.point_train_coords(keys, coarse, label, N_FG, P, K * P, N_IMP)),
        ('point_features_fwd', n_pt * (4 * C * 4 + 4 * N_FG * 4 + cin_p * 4), lambda i: ops.point_features_fwd(coords, rois_d, fmap, 0.25, coarse, N_FG, cin_p)),
        ('point_features_bwd', n_pt * (C * 4 + 2 * 4 * C * 4), lambda i: ops.point_features_bwd(g_in, coords, rois_d, 0.25, g_map)),
        ('point_concat_fwd', n_pt * (HID + N_FG + cin_p) * 4, lambda i: ops.point_concat_fwd(hid, x_in, C, N_FG, cin_p)),
        ('point_concat_bwd', n_pt * 2 * HID * 4, lambda i: ops.point_concat_bwd(g_in, HID)),
        ('point_target', n_pt * (8 + 4 + 4), lambda i: ops.point_target(masks, n_gt, rois_d, assign, label, n_pos, S, ROWS, coords)),
        ('point_bce (3 launches)', n_pt * (4 + 4) + n_pt * CP * 4, lambda i: ops.point_bce(pred, tgt, label, N_FG)),
        ('point_subdivide 28 -> 56 (D = %d)' % D, D * (784 * 4 + 3136 * 4 + 784 * 12), lambda i: ops.point_subdivide(dm, dlab, N_FG, 784)),
        ('point_subdivide 56 -> 112 (D = %d)' % D, D * (3136 * 4 + 12544 * 4 + 784 * 12), lambda i: ops.point_subdivide(g56, None, 1, 784)),
        ('point_scatter (D = %d)' % D, D * 784 * 12, lambda i: ops.point_scatter(dpred, dlab, idx2, N_FG, up2)),
    ]
    us = {name: [] for name, _, _ in cases}
    for _, _, fn in cases:
        _event_ms(fn, 5)
    for _ in range(args.reps):
        for name, _, fn in cases:
            us[name].append(_event_ms(fn, 20) * 1e3)
    return {'shape': {'batch': N, 'size': args.size, 'mask_rows': Rm, 'points': P, 'candidates': K * P, 'channels': C, 'classes': N_FG,
                      'input_channels_padded': cin_p, 'detections': D},
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
        model = MaskRCNN(n_fg_class=80, device=dev, point_rend=on)
        chain = FPNMaskRCNNTrainChain(model, mask_loss_fun=calc_mask_loss, gemm_arithmetic=DEFAULT_GEMM_ARITHMETIC)
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
    rows = [{'point_rend': name, 'step_ms_median': round(statistics.median(ms[name]), 3), 'step_ms_min': round(min(ms[name]), 3),
             'step_ms_max': round(max(ms[name]), 3), 'step_ms_all': [round(v, 3) for v in ms[name]],
             'vs_off': round(statistics.median(ms[name]) / base, 4), 'images_per_s': round(2000.0 / statistics.median(ms[name]), 2),
             'peak_allocated_MiB': round(peak[name] / 2 ** 20, 1), 'losses_finite': finite[name],
             'n_params': variants[name][1].faster_rcnn.ps.n_params()} for name in variants]
    rows[1]['peak_delta_MiB'] = round((peak['on'] - peak['off']) / 2 ** 20, 1)
    rows[1]['point_loss'] = float(variants['on'][1].observation['point_loss'])
    rows[1]['note'] = 'both models are resident in both windows: the peak is that of the process, its delta that of the PointRend step'
    return {'step': rows}


def predict_table(args, dev):
    """The mask part of ``predict`` on D fixed detections of one image's pyramid: mask branch + paste, without and with the refinement (random
    weights give no stable detection count, so the boxes are drawn here; the backbone and the box head are the same work in both)."""
    import numpy as np
    import torch
    from chainer_maskrcnn._hip import ops
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    size = args.size
    m = MaskRCNN(n_fg_class=80, device=dev, point_rend=True, min_size=size, max_size=size)
    rs = np.random.RandomState(2)
    bbox = torch.from_numpy(_boxes(rs, D, size)[:, [1, 0, 3, 2]].copy()).to(dev)
    label = torch.from_numpy(rs.randint(0, N_FG, D).astype(np.int32)).to(dev)
    level = torch.from_numpy(rs.randint(0, 4, D).astype(np.int32)).to(dev)
    img = torch.from_numpy((rs.rand(1, 3, size, size)).astype(np.float32)).to(dev)
    zeros = torch.zeros((D,), dtype=torch.int32, device=dev)

    def run(refine):
        rois5 = m._xy5(bbox)
        coarse = m.head.mask_branch(m.head.x, rois5, level, m.extractor.spatial_scales)
        if not refine:
            return ops.mask_paste(coarse, label, bbox, (size, size))
        g = m._point_refine(coarse, rois5, label)
        return ops.mask_paste(g.view(D, g.shape[1], g.shape[2], 1), zeros, bbox, (size, size))
    ms = {'off': [], 'on': []}
    with m._inference_mode():
        m.head.x = m.extractor(m.to_nhwc4(img))
        for refine in (False, True):
            for _ in range(3):
                run(refine)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, refine in (('off', False), ('on', True)):
                ms[name].append(_event_ms(lambda i: run(refine), args.steps))
    rows = [{'point_rend_refine': name, 'mask_ms_per_image_median': round(statistics.median(ms[name]), 3), 'min': round(min(ms[name]), 3),
             'max': round(max(ms[name]), 3), 'all': [round(v, 3) for v in ms[name]]} for name in ms]
    rows[1]['added_ms'] = round(statistics.median(ms['on']) - statistics.median(ms['off']), 3)
    return {'predict': {'detections': D, 'size': size, 'what': 'mask branch + paste of one image, the backbone and box head excluded', 'rows': rows}}


def run_part(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('pointrend_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(dev)}
    res.update({'kernels': kernel_table, 'step': step_table, 'predict': predict_table}[args.part](args, dev))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', default='all', choices=['all', 'kernels', 'step', 'predict'],
                    help='all: each part in a child process with its own time limit')
    ap.add_argument('--steps', type=int, default=10, help='steps per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if args.part != 'all':
        return run_part(args)
    res = {'size': args.size, 'batch': 2}
    for part in ('kernels', 'step', 'predict'):     # a fresh process per part; a part that fails or runs out of time ends the run: nothing starts after it
        cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--steps', str(args.steps), '--reps', str(args.reps), '--size', str(args.size)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=LIMITS[part], check=False)
        except subprocess.TimeoutExpired:
            raise SystemExit('pointrend_bench.py: part %r did not finish within %d s' % (part, LIMITS[part]))
        if p.returncode != 0:
            raise SystemExit('pointrend_bench.py: part %r ended with status %d' % (part, p.returncode))
        res.update(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
