#!/usr/bin/env python3
"""Device time of Soft-NMS and box voting (csrc/boxpost.hip) beside the hard class NMS on the same inputs.

Inputs: the synthetic unions of tools/tta_bench.py --mode profile - V views of 300 proposals each (V = 1, 2, 8: R = 300, 600, 2400), 81
classes, softmax of N(0, 3^2) scores, score threshold 0.05, decoded by tta_detect_decode - and the constructed worst case of the
selection loop: one class, 4096 mutually non-overlapping candidates (every one is kept: 4096 trips).

Per input, interleaved in one process (one pass over the cases per repeat, --repeats passes after --warmup): class_nms / class_nms_ws,
class_soft_nms linear and gaussian, box_vote on the hard and on the linear keep lists.  Times are hipEvent pairs around one call
(the call's launches and its output allocations), in microseconds: median and minimum over the repeats.  Prints one JSON object per
measurement; --out FILE also writes them."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SCORE_THRESH, NMS_THRESH, SIGMA, VOTE_THRESH = 0.05, 0.3, 0.5, 0.8


def union_input(V, seed=0):
    """tta_bench.py's synthetic union of V views -> (cls_bbox (300 V, 4), prob (300 V, 81)) on the device."""
    from chainer_maskrcnn._hip import ops
    R1, n_class, ld, loc0 = 300, 81, 96, 88
    rs = np.random.RandomState(seed)
    rois, box = [], []
    for v in range(V):
        c = rs.uniform(50, 550, (R1, 2)); hw = np.exp(rs.uniform(np.log(20), np.log(300), (R1, 2)))
        rois.append(torch.from_numpy(np.concatenate([c - hw / 2, c + hw / 2], 1).astype(np.float32)).cuda())
        b = np.zeros((R1, ld), np.float32)
        b[:, :n_class] = rs.standard_normal((R1, n_class)) * 3
        b[:, loc0:loc0 + 4] = rs.standard_normal((R1, 4)) * 0.5
        box.append(torch.from_numpy(b).cuda())
    mirrors = [v % 2 == 1 for v in range(V)]
    return ops.tta_detect_decode(rois, box, mirrors, [1.25] * V, n_class, loc0, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2), (480, 640))


def worst_case_input(R=4096):
    """One foreground class, R candidates on a grid of disjoint 8 x 8 boxes with distinct scores: nothing overlaps, everything is kept."""
    i = np.arange(R)
    y, x = (i // 64) * 10.0, (i % 64) * 10.0
    box = np.stack([y, x, y + 8, x + 8], 1).astype(np.float32)
    prob = np.zeros((R, 2), np.float32)
    prob[:, 1] = 0.1 + 0.8 * np.random.RandomState(1).permutation(R) / R
    return torch.from_numpy(box).cuda(), torch.from_numpy(prob).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def bench_input(name, cb, pb, l_end, args, emit):
    from chainer_maskrcnn._hip import ops
    R = int(cb.shape[0])
    hard = ops.class_nms if R <= 512 else ops.class_nms_ws
    hard_name = 'class_nms' if R <= 512 else 'class_nms_ws'
    hard_keep = hard(cb, pb, 1, l_end, SCORE_THRESH, NMS_THRESH)
    lin = ops.class_soft_nms(cb, pb, 1, l_end, SCORE_THRESH, 'linear', NMS_THRESH, SIGMA)
    gau = ops.class_soft_nms(cb, pb, 1, l_end, SCORE_THRESH, 'gaussian', NMS_THRESH, SIGMA)
    cases = [(hard_name, lambda: hard(cb, pb, 1, l_end, SCORE_THRESH, NMS_THRESH)),
             ('class_soft_nms_linear', lambda: ops.class_soft_nms(cb, pb, 1, l_end, SCORE_THRESH, 'linear', NMS_THRESH, SIGMA)),
             ('class_soft_nms_gaussian', lambda: ops.class_soft_nms(cb, pb, 1, l_end, SCORE_THRESH, 'gaussian', NMS_THRESH, SIGMA)),
             ('box_vote_on_hard', lambda: ops.box_vote(cb, pb, 1, l_end, SCORE_THRESH, VOTE_THRESH, hard_keep[0], hard_keep[1])),
             ('box_vote_on_linear', lambda: ops.box_vote(cb, pb, 1, l_end, SCORE_THRESH, VOTE_THRESH, lin[0], lin[2]))]
    kept = {hard_name: int(hard_keep[1].sum()), 'class_soft_nms_linear': int(lin[2].sum()), 'class_soft_nms_gaussian': int(gau[2].sum()),
            'box_vote_on_hard': int(hard_keep[1].sum()), 'box_vote_on_linear': int(lin[2].sum())}
    most = {hard_name: int(hard_keep[1].max()), 'class_soft_nms_linear': int(lin[2].max()), 'class_soft_nms_gaussian': int(gau[2].max())}
    times = {n: [] for n, _ in cases}
    for rep in range(args.warmup + args.repeats):
        for n, fn in cases:
            us, _ = timed(fn)
            if rep >= args.warmup:
                times[n].append(us)
    candidates = int((pb[:, 1:l_end] > SCORE_THRESH).sum())
    base = float(np.median(times[hard_name]))
    for n, _ in cases:
        t = np.asarray(times[n])
        emit({'input': name, 'rows': R, 'classes': l_end - 1, 'candidates': candidates, 'op': n, 'kept': kept[n],
              'most_kept_in_a_class': most.get(n), 'median_us': round(float(np.median(t)), 1), 'min_us': round(float(t.min()), 1),
              'ratio_to_' + hard_name: round(float(np.median(t)) / base, 2), 'repeats': args.repeats})


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--views', type=int, nargs='+', default=[1, 2, 8])
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--no-worst-case', action='store_true')
    p.add_argument('--out', default='')
    args = p.parse_args()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    with torch.no_grad():
        for V in args.views:
            cb, pb = union_input(V)
            bench_input('union_V%d' % V, cb, pb, 80, args, emit)
        if not args.no_worst_case:
            cb, pb = worst_case_input()
            bench_input('worst_case_4096_disjoint', cb, pb, 2, args, emit)
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
