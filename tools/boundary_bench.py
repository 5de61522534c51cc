#!/usr/bin/env python3
"""What Boundary AP costs on the device.  Parts, each a child process of its own with its own time limit:
  counts     device time (HIP events, median of --reps windows of --iters calls) of ops.mask_boundary_iou_counts beside ops.mask_iou_counts on
             the same inputs in the same process, windows alternating: (D, G) = (100, 20) at 375 x 500, 480 x 640 and 1024 x 1024 (d = 12,
             16, 29), rectangle-like masks and mask_paste masks; the bytes the boundary stage must move (every mask byte read once, the
             row-aligned packed rows and the packed bands written once) and their share of 8 TB/s once the per-kernel times are known.
  trace      per-kernel device times of the boundary call from a `rocprofv3 --kernel-trace --stats` run (no counters) of a child process
             that makes --trace-calls calls per shape.
  host       evaluations.mask_boundary (NumPy) on the same 120 masks, host clock, for scale.
  evaluator  InstanceSegmentationCOCOEvaluator ms per image with the metric off / on, on a fixed 100-detection stand-in for predict (the
             stand-in of tools/eval_bench.py), windows alternating.
Prints one JSON object; --out also writes it to a file.

usage: boundary_bench.py [--part all|counts|trace|host|evaluator] [--iters 20] [--reps 5] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'chainer-maskrcnn_amd'))
sys.path.insert(0, R)

HBM_PEAK = 8.0e12           # bytes/s, MI355X HBM3E
D, G = 100, 20
SHAPES = ((375, 500), (480, 640), (1024, 1024))
LIMITS = {'counts': 300, 'trace': 300, 'host': 300, 'evaluator': 300}          # seconds per part


def _rect_masks(rs, n, H, W):
    """Instance-like masks: one filled rectangle each (5..60 % of each side), at random places (tools/eval_bench.py)."""
    import numpy as np
    m = np.zeros((n, H, W), dtype=np.uint8)
    for k in range(n):
        h, w = int(H * rs.uniform(.05, .6)) + 1, int(W * rs.uniform(.05, .6)) + 1
        y, x = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        m[k, y:y + h, x:x + w] = 1
    return m


def _pasted_masks(rs, n, H, W, dev):
    """Masks as predict() makes them: smooth random 28 x 28 logits pasted into random boxes by ops.mask_paste."""
    import numpy as np
    import torch
    from chainer_maskrcnn._hip import ops
    S, Cm = 28, 96
    yy, xx = np.mgrid[0:S, 0:S] / float(S)
    logits = np.zeros((n, S, S, Cm), np.float32)
    for k in range(n):
        cy, cx, ry, rx = rs.uniform(.35, .65), rs.uniform(.35, .65), rs.uniform(.2, .45), rs.uniform(.2, .45)
        logits[k, :, :, 0] = 4.0 * (1.0 - ((yy - cy) / ry) ** 2 - ((xx - cx) / rx) ** 2) + rs.standard_normal((S, S)) * 0.3
    h, w = H * rs.uniform(.05, .6, n) + 1, W * rs.uniform(.05, .6, n) + 1
    y, x = rs.uniform(0, 1, n) * (H - h), rs.uniform(0, 1, n) * (W - w)
    bbox = np.stack([y, x, y + h, x + w], 1).astype(np.float32)
    return ops.mask_paste(torch.from_numpy(logits).to(dev), torch.zeros((n,), dtype=torch.int32, device=dev), torch.from_numpy(bbox).to(dev),
                          (H, W))


def _inputs(dev):
    """[(kind, H, W, a (D,H,W), b (G,H,W), labels a, labels b)] on the device."""
    import numpy as np
    import torch
    rs = np.random.RandomState(0)
    out = []
    for H, W in SHAPES:
        la = torch.from_numpy(rs.randint(0, 80, D).astype(np.int32)).to(dev)
        lb = torch.from_numpy(rs.randint(0, 80, G).astype(np.int32)).to(dev)
        out.append(('rectangles', H, W, torch.from_numpy(_rect_masks(rs, D, H, W)).to(dev), torch.from_numpy(_rect_masks(rs, G, H, W)).to(dev), la, lb))
        out.append(('mask_paste', H, W, _pasted_masks(rs, D, H, W, dev), _pasted_masks(rs, G, H, W, dev), la, lb))
    return out


def _event_us(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def stage_bytes(H, W, n=D + G):
    """Bytes the boundary stage must move for n masks: each mask byte read once, the packed rows and the packed bands written once."""
    row_words = (W + 63) // 64
    return {'mask_bytes_read': n * H * W, 'packed_rows_written': n * H * row_words * 8, 'packed_bands_written': n * H * row_words * 8}


def counts_table(args, dev):
    from chainer_maskrcnn import evaluations
    from chainer_maskrcnn._hip import ops
    rows = []
    for kind, H, W, a, b, la, lb in _inputs(dev):
        for labels in (False, True):
            extra = (la, lb) if labels else ()
            plain = lambda: ops.mask_iou_counts(a, b, *extra)
            bound = lambda: ops.mask_boundary_iou_counts(a, b, *extra)
            for fn in (plain, bound):
                _event_us(fn, 5)
            us = {'plain': [], 'boundary': []}
            for _ in range(args.reps):
                us['plain'].append(_event_us(plain, args.iters))
                us['boundary'].append(_event_us(bound, args.iters))
            mp, mb = statistics.median(us['plain']), statistics.median(us['boundary'])
            nbytes = stage_bytes(H, W)
            rows.append({'masks': kind, 'H': H, 'W': W, 'D': D, 'G': G, 'dilation': evaluations.boundary_dilation(H, W), 'labels': labels,
                         'mask_iou_counts_us': round(mp, 2), 'mask_iou_counts_us_all': [round(v, 2) for v in us['plain']],
                         'mask_boundary_iou_counts_us': round(mb, 2), 'mask_boundary_iou_counts_us_all': [round(v, 2) for v in us['boundary']],
                         'ratio': round(mb / mp, 3), 'stage_bytes': nbytes, 'stage_bytes_total': sum(nbytes.values()),
                         'note': 'through the Python wrapper: output and workspace allocation and the ctypes call are in the window'})
    return {'counts': rows}


def trace_child(args, dev):
    """The program rocprofv3 wraps: --trace-calls boundary calls per input, nothing timed here."""
    import torch
    from chainer_maskrcnn._hip import ops
    for kind, H, W, a, b, la, lb in _inputs(dev):
        if kind != args.trace_kind or (H, W) != tuple(args.trace_shape):
            continue
        for _ in range(args.trace_calls):
            ops.mask_boundary_iou_counts(a, b)
    torch.cuda.synchronize()
    return {}


def trace_table(args, dev):
    """Per-kernel average times of the boundary call, one profiled child process per (masks, shape): the kernels of different shapes share
    their names, so each shape gets its own statistics."""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    rows = []
    for kind in ('rectangles', 'mask_paste'):
        for H, W in SHAPES:
            out = tempfile.mkdtemp(prefix='boundary_bench_')
            cmd = [prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'b', '--', sys.executable, os.path.abspath(__file__),
                   '--part', 'trace-child', '--trace-kind', kind, '--trace-shape', str(H), str(W), '--trace-calls', str(args.trace_calls)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
            files = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
            if r.returncode != 0 or not files:
                raise SystemExit('boundary_bench.py: rocprofv3 ended with status %d and %d stats files: %s'
                                 % (r.returncode, len(files), r.stdout.decode('utf-8', 'replace')[-300:]))
            stats = {}
            for row in csv.DictReader(open(files[0])):
                name = re.search(r'\bk_mask_[A-Za-z0-9_]+', row.get('Name', ''))
                if name:
                    calls = int(row['Calls'])
                    avg = float(row['AverageNs']) if row.get('AverageNs') else float(row['TotalDurationNs']) / calls
                    stats[name.group(0)] = {'launches_per_call': calls / float(args.trace_calls), 'avg_us': round(avg / 1e3, 2)}
            shutil.rmtree(out, ignore_errors=True)
            nbytes = stage_bytes(H, W)
            stage_us = sum(stats[k]['avg_us'] for k in ('k_mask_pack_rows', 'k_mask_boundary') if k in stats)
            rows.append({'masks': kind, 'H': H, 'W': W, 'kernels': stats, 'boundary_stage_us': round(stage_us, 2),
                         'stage_bytes_total': sum(nbytes.values()),
                         'stage_share_of_hbm_peak': round(sum(nbytes.values()) / (stage_us * 1e-6) / HBM_PEAK, 4) if stage_us else None,
                         'pack_rows_share_of_hbm_peak': round((nbytes['mask_bytes_read'] + nbytes['packed_rows_written'])
                                                              / (stats['k_mask_pack_rows']['avg_us'] * 1e-6) / HBM_PEAK, 4)
                         if 'k_mask_pack_rows' in stats else None})
    return {'trace': {'calls_per_shape': args.trace_calls, 'includes_first_call': True, 'rows': rows}}


def host_table(args, dev):
    import numpy as np
    from chainer_maskrcnn import evaluations
    rs = np.random.RandomState(0)
    rows = []
    for H, W in SHAPES:
        m = _rect_masks(rs, D + G, H, W)
        d = evaluations.boundary_dilation(H, W)
        t0 = time.perf_counter()
        band = evaluations.mask_boundary(m, d)
        rows.append({'H': H, 'W': W, 'masks': D + G, 'dilation': d, 'numpy_mask_boundary_ms': round((time.perf_counter() - t0) * 1e3, 1),
                     'band_pixels': int(band.sum())})
    return {'host': rows}


class _FixedTarget(object):
    """predict() returns the same device-resident (D, H, W) masks, labels and scores for every image: the evaluator's own cost."""

    def __init__(self, masks, labels, scores, boxes):
        self.out, self.train, self.device, self.last_bboxes = ([masks], [labels], [scores]), True, masks.device, [boxes]

    def predict(self, imgs):
        return self.out


def evaluator_table(args, dev):
    import numpy as np
    import torch
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, SyntheticCOCOEvalDataset
    rows = []
    for H, W in ((480, 640), (1024, 1024)):
        rs = np.random.RandomState(1)
        data = SyntheticCOCOEvalDataset(args.images, H, W, n_fg_class=80)
        examples = [data[i] for i in range(len(data))]
        boxes = torch.from_numpy(np.tile(np.array([[0, 0, H, W]], np.float32), (D, 1))).to(dev)
        fixed = _FixedTarget(torch.from_numpy(_rect_masks(rs, D, H, W)).to(dev), torch.from_numpy(rs.randint(0, 80, D).astype(np.int32)).to(dev),
                             torch.from_numpy(rs.rand(D).astype(np.float32)).to(dev), boxes)
        types = {'off': ('segm', 'bbox'), 'on': ('segm', 'bbox', 'boundary')}

        def once(name):
            ev = InstanceSegmentationCOCOEvaluator(examples, fixed, cat_ids=data.cat_ids, iou_types=types[name])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / len(examples)
        for name in types:
            once(name)
        ms = {name: [] for name in types}
        for _ in range(args.reps):
            for name in types:
                ms[name].append(once(name))
        rows.append({'H': H, 'W': W, 'images': len(examples), 'detections_per_image': D, 'gt_per_image': 8,
                     'ms_per_image_off': round(statistics.median(ms['off']), 3), 'ms_per_image_on': round(statistics.median(ms['on']), 3),
                     'off_all': [round(v, 3) for v in ms['off']], 'on_all': [round(v, 3) for v in ms['on']],
                     'note': 'host clock over evaluate(): the matching and the summary (a third accumulator when on) are inside'})
    return {'evaluator': rows}


PARTS = {'counts': counts_table, 'trace': trace_table, 'host': host_table, 'evaluator': evaluator_table, 'trace-child': trace_child}


def run_part(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('boundary_bench.py measures on a HIP device; none found')
    dev = torch.device('cuda:0')
    res = PARTS[args.part](args, dev)
    if args.part != 'trace-child':
        res['device'] = torch.cuda.get_device_name(dev)
        print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', default='all', choices=['all'] + sorted(PARTS), help='all: each part in a child process with its own time limit')
    ap.add_argument('--iters', type=int, default=20, help='calls per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per variant (interleaved); the median is reported')
    ap.add_argument('--images', type=int, default=8, help='images of the evaluator part')
    ap.add_argument('--trace-calls', type=int, default=20)
    ap.add_argument('--trace-kind', default='rectangles', help=argparse.SUPPRESS)
    ap.add_argument('--trace-shape', type=int, nargs=2, default=[1024, 1024], help=argparse.SUPPRESS)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if args.part != 'all':
        return run_part(args)
    res = {'D': D, 'G': G}
    for part in ('counts', 'trace', 'host', 'evaluator'):     # a fresh process per part; a part that fails or runs out of time ends the run
        cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--iters', str(args.iters), '--reps', str(args.reps),
               '--images', str(args.images), '--trace-calls', str(args.trace_calls)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=LIMITS[part], check=False)
        except subprocess.TimeoutExpired:
            raise SystemExit('boundary_bench.py: part %r did not finish within %d s' % (part, LIMITS[part]))
        if p.returncode != 0:
            raise SystemExit('boundary_bench.py: part %r ended with status %d' % (part, p.returncode))
        res.update(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
