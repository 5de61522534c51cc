"""The hand-made Copy-Paste batch of tests/test_copy_paste_cpu.py and tests/test_copy_paste_gpu.py: three examples of three
rows on an H x W canvas, as the large-scale-jitter stage leaves them (kept rows first, `gather` = the identity on them).
  example 0  receives; offers everything.  A0 = rows 4..19, columns 4..19, label 1; A1 = rows 30..39, columns 30..39, label 2; one empty row
  example 1  receives; B0 = rows 0..25, columns 0..25, label 3, offered; B1 = rows 35..50, columns 20..45, label 4, offered; B2 = the last 4
             rows and columns, label 5, NOT offered
  example 2  does not receive and offers nothing: one instance, rows 10..12, columns 33..W-1, label 6
Pasting example 1 onto example 0 covers A0 (dropped) and the lower half of A1 (its box shrinks to rows 30..34)."""
import numpy as np

# the shapes of tests/test_lsj_gpu.py, one block per plane in the mask kernels; the second has ragged rows (W % 16 != 0, W % 4 != 0).  The
# canvases of several blocks per plane - 128 x 128, 100 x 208, 100 x 200 (W % 4 == 0 only) - are tests/augment_edge_cases.py's
CANVASES = [(64, 64), (61, 50)]


def rect(H, W, ys, xs):
    """ys, xs: first and last row / column, inclusive."""
    m = np.zeros((H, W), np.uint8)
    m[ys[0]:ys[1] + 1, xs[0]:xs[1] + 1] = 1
    return m


def handmade(canvas):
    """(batch as loader.collate gives it, gather (3,3) int32, sel (3,3) uint8, receive (3,) uint8)."""
    H, W = canvas
    rs = np.random.RandomState(7)
    zero = np.zeros((H, W), np.uint8)
    masks = np.stack([np.stack([rect(H, W, (4, 19), (4, 19)), rect(H, W, (30, 39), (30, 39)), zero]),
                      np.stack([rect(H, W, (0, 25), (0, 25)), rect(H, W, (35, 50), (20, 45)), rect(H, W, (H - 4, H - 1), (W - 4, W - 1))]),
                      np.stack([rect(H, W, (10, 12), (33, W - 1)), zero, zero])])
    labels = np.array([[1, 2, -1], [3, 4, 5], [6, -1, -1]], np.int32)
    bboxes = np.zeros((3, 3, 4), np.float32)
    for n in range(3):
        for g in range(3):
            ys, xs = np.nonzero(masks[n, g])
            if len(ys):
                bboxes[n, g] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    batch = {'imgs': rs.rand(3, 3, H, W).astype(np.float32), 'masks': masks, 'labels': labels, 'bboxes': bboxes,
             'scales': np.array([1.0, 0.5, 2.0], np.float32), 'sizes': np.array([[40, W], [H, 46], [13, W]], np.float32)}
    gather = np.where(labels >= 0, np.arange(3, dtype=np.int32)[None], -1).astype(np.int32)
    sel = np.array([[1, 1, 1], [1, 1, 0], [0, 0, 0]], np.uint8)
    receive = np.array([1, 1, 0], np.uint8)
    return batch, gather, sel, receive


def offers_of(gather, sel):
    """Per example, which batch rows are offered: the row's original instance index looked up in sel (rows without one: not offered)."""
    return [np.array([g >= 0 and bool(s[g]) for g in gs]) for gs, s in zip(gather, sel)]
