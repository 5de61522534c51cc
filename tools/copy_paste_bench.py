#!/usr/bin/env python3
"""Device time of the Copy-Paste stage beside the large-scale-jitter assembly it follows, per batch, with HIP events
over many batches:
  lsj        the yardstick: the LSJ assembly of lsj_bench.py's case lsj_s1 (image writer, box / compaction launches, mask writer), in
             this process
  cp_image   mrcnn_copy_paste_image_f32 on the LSJ batch: alpha plane + composed image, one launch
  cp_masks   mrcnn_copy_paste_masks_u8: one fill, the reduce pass over the G + G candidate rows, finalize, the mask writer
  cp         both calls, as ops.copy_paste issues them (its allocations included)
  lsj_cp     the LSJ assembly followed by ops.copy_paste, as the loader issues them
Batch size 2, the sources and instance masks of lsj_bench.py (640 x 480 / 427 x 640, --gt instances each), S = 1024, s = 1; every
example receives and offers every other instance; G_out = 2 x gt, what the loader asks for without --max-gt.  Sources already on the
device.  Two alternating repeats in one process: the spread between them shows the noise.  --per-launch 1 adds the average time of each
kernel from a kernel trace of a child process (rocprofv3 --kernel-trace --stats over --trace-batches batches of lsj_cp).  Prints one JSON
line."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def kernel_trace(a):
    """Average ns per kernel of a child process that runs lsj_cp --trace-batches times under rocprofv3 (a fresh process: the profiler
    wraps the program from its start)."""
    out = tempfile.mkdtemp(prefix='copy_paste_bench_')
    cmd = [shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'cp',
           '--', sys.executable, os.path.abspath(__file__), '--trace-child', '1', '--batches', str(a.trace_batches), '--warmup', '0',
           '--gt', str(a.gt), '--size', str(a.size)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    files = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if r.returncode != 0 or not files:
        return {'error': 'rocprofv3 exit %d, %d stats files: %s' % (r.returncode, len(files), r.stdout.decode('utf-8', 'replace')[-300:])}
    stats = {}
    for row in csv.DictReader(open(files[0])):          # (names come as "(anonymous namespace)::k_cp_compose(float const*, ...)")
        name = re.search(r'\bk_[A-Za-z0-9_]+', row.get('Name', ''))
        if name:
            calls = int(row['Calls'])
            avg = float(row['AverageNs']) if row.get('AverageNs') else float(row['TotalDurationNs']) / calls
            stats[name.group(0)] = {'calls': calls, 'avg_us': round(avg / 1e3, 2)}
    return stats


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--gt', type=int, default=8)
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--per-launch', type=int, default=0, choices=[0, 1])
    p.add_argument('--trace-batches', type=int, default=20)
    p.add_argument('--trace-child', type=int, default=0, choices=[0, 1], help=argparse.SUPPRESS)
    a = p.parse_args()
    from chainer_maskrcnn import _hip
    from chainer_maskrcnn._hip import ops, ptr, stream_ptr
    from chainer_maskrcnn.dataset.augment import lsj_geometry
    if not torch.cuda.is_available():
        raise SystemExit('copy_paste_bench.py needs a HIP device')
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    srcs = [(480, 640), (640, 427)]
    imgs = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in srcs]
    masks = [(rs.rand(a.gt, H, W) > 0.5).astype(np.uint8) for H, W in srcs]
    img_pack = torch.from_numpy(np.concatenate([x.reshape(-1) for x in imgs])).to(dev)
    mask_pack = torch.from_numpy(np.concatenate([x.reshape(-1) for x in masks])).to(dev)
    img_offs = np.cumsum([0] + [x.nbytes for x in imgs])[:-1]
    mask_offs = np.cumsum([0] + [x.nbytes for x in masks])[:-1]
    N, G, S = len(srcs), a.gt, a.size
    G_out = 2 * G
    flips = [i % 2 for i in range(N)]
    labels_in = torch.arange(N * G, dtype=torch.int32, device=dev).reshape(N, G)
    geos = [lsj_geometry(H, W, S, 1.0, 0.5, 0.5) for H, W in srcs]
    d = ops.crop_descs([(o, H, W, g[0], g[1], f, 0) + g[2:] for o, (H, W), g, f in zip(img_offs, srcs, geos, flips)])
    md = ops.crop_descs([(o, H, W, g[0], g[1], f, G) + g[2:] for o, (H, W), g, f in zip(mask_offs, srcs, geos, flips)])
    sel = torch.from_numpy(np.tile((np.arange(G) % 2 == 0).astype(np.uint8), (N, 1))).to(dev)
    receive = torch.ones((N,), dtype=torch.uint8, device=dev)

    def lsj():
        im = ops.image_resize_crop_batch_u8(img_pack, d, S, S, 255.0)
        bb, lab, gather = ops.mask_crop_boxes_u8(mask_pack, md, labels_in, G, S, S)
        return im, ops.mask_resize_crop_batch_u8(mask_pack, md, gather, S, S), lab, gather

    def lsj_cp():
        im, m, lab, gather = lsj()
        return ops.copy_paste(im, m, lab, gather, sel, receive, G_out)

    if a.trace_child:
        for _ in range(a.batches):
            lsj_cp()
        torch.cuda.synchronize()
        return
    im, m, lab, gather = lsj()
    out_imgs, alpha = torch.empty_like(im), torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    out_masks = torch.empty((N, G_out, S, S), dtype=torch.uint8, device=dev)
    bboxes, out_labels = torch.empty((N, G_out, 4), device=dev), torch.empty((N, G_out), dtype=torch.int32, device=dev)
    source, ws = torch.empty((N, G_out), dtype=torch.int32, device=dev), torch.empty((N, 2 * G, 4), dtype=torch.int32, device=dev)
    lib = _hip.lib()

    def cp_image():
        _hip.check(lib.mrcnn_copy_paste_image_f32(ptr(im), ptr(m), ptr(lab), ptr(gather), ptr(sel), ptr(receive), N, G, G, S, S, ptr(out_imgs),
                                                  ptr(alpha), stream_ptr()))

    def cp_masks():
        _hip.check(lib.mrcnn_copy_paste_masks_u8(ptr(m), ptr(alpha), ptr(lab), ptr(gather), ptr(sel), ptr(receive), N, G, G, G_out, S, S,
                                                 ptr(out_masks), ptr(bboxes), ptr(out_labels), ptr(source), ptr(ws), stream_ptr()))

    stages = {'lsj': lsj, 'cp_image': cp_image, 'cp_masks': cp_masks, 'cp': lambda: ops.copy_paste(im, m, lab, gather, sel, receive, G_out),
              'lsj_cp': lsj_cp}
    # same bits: the two calls on their own buffers against the op
    cp_image()
    cp_masks()
    want = stages['cp']()
    assert all(torch.equal(x, y) for x, y in zip((out_imgs, out_masks, bboxes, out_labels), want)), 'the calls and the op differ'
    kept = int((want[3] >= 0).sum())
    pasted_share = float((alpha != 0).float().mean())

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batches

    res = {}
    for rep in range(2):
        for k, fn in stages.items():
            res.setdefault(k + '_ms', []).append(timed(fn))
    px = N * S * S
    # compose: own image in and out, the pasted share of the partner's, the offered planes in, alpha out; reduce: the valid own planes
    # + alpha per plane + the picked partner planes; writer: one plane (+ alpha for own rows) in per kept row, G_out planes out
    picked = G // 2 + G % 2
    moved = {'cp_image': px * (24 + 12 * pasted_share + picked + 1), 'cp_masks': px * ((2 * G + picked) + (2 * kept / N - picked) + G_out)}
    moved['cp'] = moved['cp_image'] + moved['cp_masks']
    line = {'metric': 'ms per bs-2 batch (device time, HIP events)', 'batches': a.batches, 'gt_per_image': G, 'G_out': G_out, 'sources': srcs,
            'canvas': S, 'geometry': [list(g) for g in geos], 'kept_rows': kept, 'pasted_share_of_canvas': round(pasted_share, 4),
            'bytes_moved_per_batch': {k: int(v) for k, v in moved.items()}}
    line.update({k: [round(t, 4) for t in v] for k, v in res.items()})
    line['TBps'] = {k: round(v / (min(res[k + '_ms']) * 1e-3) / 1e12, 3) for k, v in moved.items()}
    line['note'] = ('TBps = bytes moved / device time; the loop re-reads one batch, which largely stays in the 256 MB Infinity Cache: not '
                    'an HBM rate')
    line['cp_over_lsj'] = round(min(res['cp_ms']) / min(res['lsj_ms']), 2)
    if a.per_launch:
        line['per_launch'] = kernel_trace(a)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
