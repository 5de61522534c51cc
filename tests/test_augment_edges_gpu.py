"""The augmentation kernels past one workgroup per plane, one ballot round per example and one pass of picked rows (csrc/augment.hip,
csrc/copy_paste.hip), through ops.* against the NumPy rules: resize_linear / resize_nearest sliced and
tight boxes for large-scale jitter, augment.copy_paste_batch for Copy-Paste.  Every output is a selection, an integer max or a fixed
float expression, so every comparison is exact.

Cases.  tests/augment_edge_cases.py builds them and restates the thread map (16 bytes a thread, 256 threads a block, 64 candidates a
ballot round, 256 picked rows a pass); tests/test_augment_edge_cases_cpu.py holds every case against the path it is named for, without a
device.  The older GPU tests run 64 x 64 and 61 x 50 canvases - one block per plane - with at most 7 instances; here the planes take 2 to
6 blocks (a block starting inside a row, a partly idle last block, blocks below a short window), the finalize kernels walk up to 9
rounds of candidates with the truncation inside, at the start of and in front of a later round, Copy-Paste takes G = 257 rows, mask
bytes other than 1, views that are not 16-byte aligned and batches where nothing is pasted, and the LSJ kernels take all 32 descriptors.
The device loader runs against the host loader on a 128 canvas.

What each test holds, and a wrong variant that tests/test_lsj_gpu.py and tests/test_copy_paste_gpu.py pass (one block, one round, one
pass: the variant computes the same there) and this file rejects:
  box extremes, multi-block Copy-Paste   `atomicMax(&ws[...], m)` of k_mask_crop_reduce / k_cp_reduce - a plain store keeps one block's
                                         maxima; `i = blockIdx.x * NT + threadIdx.x` of the writers k_mask_resize_batch_u8 / k_cp_masks -
                                         without the block offset every block writes the first 256 threads' rows
  short window                           `(blockIdx.x * NT) / wq >= win.ch` and `y < win.ch` of k_mask_crop_reduce - an exit test on the
                                         block's last row would drop the block that straddles the window's end
  ballot rounds, candidates past a wave  `kept += __popcll(m)`, `pos = kept + ...` and `pos < G` / `pos < G_out` of k_mask_crop_finalize /
                                         k_cp_finalize - with `kept` not carried a later round overwrites the rows of the first
  G = 257                                `base + k` in k_cp_compose's plane index - without `base` the second pass reads row 0 for row 256
  byte values                            nonzero_bytes - a test of bit 0 misses 2 and 128
  misaligned views                       `vec` = 0 with W % 16 == 0 in both entry points - the byte rows
  full batches                           32 descriptors by value in all five LSJ / resize kernels - a table cut at fewer entries"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.dataset.augment import Augment, copy_paste_batch, lsj_geometry  # noqa: E402
from chainer_maskrcnn.dataset.loader import BatchLoader, collate  # noqa: E402
from chainer_maskrcnn.dataset.transforms import RawTransform, Transform, resize_nearest  # noqa: E402
from tests import augment_edge_cases as cases  # noqa: E402
from tests.augment_data import write_coco  # noqa: E402
from tests.augment_edge_cases import CANVAS_IDS, CANVASES, np_copy_paste, np_lsj  # noqa: E402

DEV = 'cuda:0'
FLIPS = pytest.mark.parametrize('flip', [0, 1], ids=['unflipped', 'flipped'])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _upload(arrays):
    buf, offs = cases.pack(arrays)
    return _dev(buf), offs


# ---- large-scale jitter: boxes, compaction and the gathering mask writer ------------------------------------------------------------------
def _lsj(batch, G, canvas):
    """mask_crop_boxes_u8, then the mask writer on the table it made."""
    src, offs = _upload([m for m, _, _ in batch])
    desc = ops.crop_descs(cases.mask_rows(batch, offs))
    bboxes, labels, gather = ops.mask_crop_boxes_u8(src, desc, _dev(cases.labels_of(batch)), G, canvas[0], canvas[1])
    masks = ops.mask_resize_crop_batch_u8(src, desc, gather, canvas[0], canvas[1])
    assert bboxes.dtype == torch.float32 and labels.dtype == torch.int32 and gather.dtype == torch.int32 and masks.dtype == torch.uint8
    return {'gather': gather.cpu().numpy(), 'labels': labels.cpu().numpy(), 'bboxes': bboxes.cpu().numpy(), 'masks': masks.cpu().numpy()}


def _check_lsj(batch, G, canvas):
    got, want = _lsj(batch, G, canvas), np_lsj(batch, G, canvas)
    for k in ('gather', 'labels', 'bboxes', 'masks'):
        assert got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s, G = %d' % (k, G))
    return got


@FLIPS
@pytest.mark.parametrize('canvas', CANVASES, ids=CANVAS_IDS)
def test_box_extremes_in_different_blocks_meet_in_the_workspace(canvas, flip):
    H, W = canvas
    got = _check_lsj(cases.extremes_case(canvas, flip), 5, canvas)
    np.testing.assert_array_equal(got['bboxes'][0, :2], [[0, 0, H, W], [H - 1, W - 1, H, W]])


@FLIPS
@pytest.mark.parametrize('name', sorted(cases.WINDOW_CASES))
def test_window_shorter_than_the_canvas(name, flip):
    canvas, ch = cases.WINDOW_CASES[name]
    batch = cases.window_case(name, flip)
    got = _check_lsj(batch, batch[0][0].shape[0], canvas)
    assert (got['labels'][0] >= 0).sum() == 4 and not got['masks'][0, :, ch:].any()


@FLIPS
def test_more_than_one_ballot_round(flip):
    batch = cases.ballot_case(flip)
    for G in cases.BALLOT_GS:
        got = _check_lsj(batch, G, cases.BALLOT_CANVAS)
        assert (got['labels'][0] >= 0).sum() == min(G, 125) and got['gather'][1, 0] == 64


@FLIPS
def test_a_full_batch_of_crop_descriptors(flip):
    H, W = cases.MANY_CANVAS
    imgs, batch = cases.many_case(True, flip)
    _check_lsj(batch, 3, cases.MANY_CANVAS)
    examples = [(i, f, g) for i, (_, f, g) in zip(imgs, batch)]
    src, offs = _upload(imgs)
    out = ops.image_resize_crop_batch_u8(src, ops.crop_descs(cases.image_rows(examples, offs)), H, W, 255.0).cpu().numpy()
    np.testing.assert_array_equal(out, cases.np_images(examples, cases.MANY_CANVAS))
    assert out[31].any()


@FLIPS
def test_a_full_batch_of_resize_descriptors(flip):
    H, W = cases.MANY_CANVAS
    imgs, batch = cases.many_case(False, flip)
    examples = [(i, f, g) for i, (_, f, g) in zip(imgs, batch)]
    src, offs = _upload(imgs)
    out = ops.image_resize_batch_u8(src, ops.resize_descs([r[:7] for r in cases.image_rows(examples, offs)]), H, W, 255.0).cpu().numpy()
    np.testing.assert_array_equal(out, cases.np_images(examples, cases.MANY_CANVAS))
    msrc, moffs = _upload([m for m, _, _ in batch])
    got = ops.mask_resize_batch_u8(msrc, ops.resize_descs([r[:7] for r in cases.mask_rows(batch, moffs)]), 3, H, W).cpu().numpy()
    want = np.zeros((len(batch), 3, H, W), np.uint8)
    for n, (m, f, (oh, ow, _, _, _, _)) in enumerate(batch):
        for k in range(m.shape[0]):
            want[n, k, :oh, :ow] = resize_nearest(m[k][:, ::-1] if f else m[k], (oh, ow))
    np.testing.assert_array_equal(got, want)
    assert got[31, 2].any() and out[31].any()


@FLIPS
@pytest.mark.parametrize('canvas', CANVASES, ids=CANVAS_IDS)
def test_image_crop_writer_on_the_multi_block_canvases(canvas, flip):
    """(100, 200): float4 image rows beside byte-stored mask rows."""
    examples = cases.image_case(canvas, flip)
    src, offs = _upload([e[0] for e in examples])
    out = ops.image_resize_crop_batch_u8(src, ops.crop_descs(cases.image_rows(examples, offs)), canvas[0], canvas[1], 255.0).cpu().numpy()
    np.testing.assert_array_equal(out, cases.np_images(examples, canvas))
    assert np.count_nonzero(out[1, :, 45:]) == 0 and np.count_nonzero(out[1, :, :, 63:]) == 0 and np.count_nonzero(out[1]) > 0


# ---- Copy-Paste ------------------------------------------------------------------------------------------------------------------------------
def _copy_paste(case, G_out, given=None):
    batch, gather, sel, receive = case
    given = given or [_dev(batch['imgs']), _dev(batch['masks'])]
    given = given + [_dev(batch['labels']), _dev(gather), _dev(sel), _dev(receive)]
    before = [g.clone() for g in given]
    imgs, masks, bboxes, labels = ops.copy_paste(*given, G_out)
    for g, b in zip(given, before):                          # the pre-paste batch is only read
        assert torch.equal(g, b)
    assert imgs.dtype == torch.float32 and masks.dtype == torch.uint8 and bboxes.dtype == torch.float32 and labels.dtype == torch.int32
    return {'imgs': imgs.cpu().numpy(), 'masks': masks.cpu().numpy(), 'bboxes': bboxes.cpu().numpy(), 'labels': labels.cpu().numpy()}


def _check(got, want, what=''):
    for k in ('labels', 'bboxes', 'masks', 'imgs'):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (k, what))


@pytest.mark.parametrize('N', [2, 3])
@pytest.mark.parametrize('canvas', CANVASES, ids=CANVAS_IDS)
def test_copy_paste_on_the_multi_block_canvases(canvas, N):
    case = cases.cp_multiblock(canvas, N)
    for G_out in (8, 3):                                     # room for every row; truncation
        _check(_copy_paste(case, G_out), np_copy_paste(case, G_out), 'G_out = %d' % G_out)


@pytest.mark.parametrize('G', cases.WAVE_GS)
def test_copy_paste_candidates_past_one_wave(G):
    case = cases.cp_waves(G)
    for G_out in cases.wave_g_outs(G):
        _check(_copy_paste(case, G_out), np_copy_paste(case, G_out), 'G_out = %d' % G_out)


def test_copy_paste_with_more_rows_than_one_pass_of_picks():
    case = cases.cp_many_rows()
    want = np_copy_paste(case, cases.MANY_ROWS_G_OUT)
    got = _copy_paste(case, cases.MANY_ROWS_G_OUT)
    _check(got, want)
    assert got['labels'][0, 256] == 1257 and got['labels'][1, 256:260].tolist() == [4, 101, 256, 257]    # the pasted rows, behind the own ones


@pytest.mark.parametrize('canvas', [CANVASES[0], CANVASES[2]], ids=[CANVAS_IDS[0], CANVAS_IDS[2]])
def test_copy_paste_keeps_the_byte_values(canvas):
    case = cases.cp_byte_values(canvas)
    got = _copy_paste(case, 8)
    _check(got, np_copy_paste(case, 8))
    assert set(got['masks'].reshape(-1)) == {0, 1, 2, 128, 255}


def test_copy_paste_on_views_that_are_not_16_byte_aligned():
    """W % 16 == 0 with a base pointer off the 16-byte grid: the entry points fall back to the byte / scalar rows."""
    case = cases.cp_multiblock((128, 128), 3)
    batch = case[0]
    want = np_copy_paste(case, 8)
    aligned = _copy_paste(case, 8)
    _check(aligned, want)

    def view(a, skip):                                       # a contiguous view `skip` elements into a larger buffer
        buf = torch.empty((a.size + 16,), dtype=torch.from_numpy(a).dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[skip:skip + a.size].view(a.shape)
        v.copy_(_dev(a))
        assert v.is_contiguous() and v.data_ptr() % 16 == skip * a.itemsize
        return v

    for skip_imgs, skip_masks in ((0, 1), (1, 0), (1, 1)):   # masks at byte offset 1, images at byte offset 4
        got = _copy_paste(case, 8, [view(batch['imgs'], skip_imgs), view(batch['masks'], skip_masks)])
        _check(got, want, 'offsets %d / %d' % (skip_imgs, skip_masks))
        _check(got, aligned)


@pytest.mark.parametrize('kind', ['receive', 'sel'])
def test_copy_paste_with_nothing_to_paste(kind):
    case = cases.cp_no_paste(kind)
    batch = case[0]
    got = _copy_paste(case, 4)
    _check(got, np_copy_paste(case, 4))
    np.testing.assert_array_equal(got['imgs'], batch['imgs'])
    np.testing.assert_array_equal(got['masks'][:2], batch['masks'][:2, :4])
    assert got['labels'][2].tolist() == [9, 11, -1, -1]      # the empty row is gone


# ---- the device loader against the host loader on a 128 canvas: 4 blocks per plane, where the 64 canvas of the older tests has one ------------
class _Sizes(object):
    min_size, max_size = 96, 160


LOADER_S, LOADER_BATCHES = 128, 4
LOADER_SEED = 4     # chosen on the CPU, with the host rule: see the assertions in front of the comparisons
LOADER_SIZES = [(97, 131), (120, 100), (91, 157), (128, 128), (101, 99)]


def _dataset(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader
    root = write_coco(str(tmp_path), n_img=5, sizes=LOADER_SIZES)
    ds = COCOMaskLoader(anno_dir=root + '/annotations', img_dir=root, split='train', data_type='2017')
    order = np.concatenate([np.random.RandomState(2 + e).permutation(len(ds)) for e in range(3)])       # BatchLoader(shuffle=True, seed=2)
    return ds, order


def _compare(ds, aug, max_gt):
    kw = dict(batch_size=2, shuffle=True, seed=2, num_workers=2, max_gt=max_gt, device=DEV, augment=aug)
    host, devl = BatchLoader(ds, Transform(_Sizes()), **kw), BatchLoader(ds, RawTransform(_Sizes()), **kw)
    try:
        for _ in range(LOADER_BATCHES):
            a, b = next(host), next(devl)
            for k in ('imgs', 'masks', 'bboxes', 'labels', 'scales', 'sizes'):
                x, y = a[k], b[k]
                x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
                y = y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
                if max_gt is None and k in ('masks', 'bboxes', 'labels') and y.shape[1] > x.shape[1]:
                    # without max_gt the device path sizes its rows by the instances BEFORE the crop (it does not wait for the kept
                    # counts); the host sizes them by the kept ones: the device's extra rows are empty
                    g = x.shape[1]
                    assert (y[:, g:] == (-1 if k == 'labels' else 0)).all(), k
                    y = y[:, :g]
                assert x.dtype == y.dtype and x.shape == y.shape, k
                np.testing.assert_array_equal(x, y, err_msg=k)
            assert tuple(b['imgs'].shape[2:]) == (LOADER_S, LOADER_S) and cases.blocks(LOADER_S, LOADER_S) == 4
    finally:
        host.close()
        devl.close()


@pytest.mark.parametrize('max_gt', [3, None])
def test_lsj_device_loader_equals_host_transform_on_a_multi_block_canvas(tmp_path, max_gt):
    from chainer_maskrcnn.dataset.augment import hflip
    ds, order = _dataset(tmp_path)
    aug = Augment(hflip_prob=0.5, seed=LOADER_SEED, lsj_size=LOADER_S)
    # what the batches hold, by the host rule: an instance the window cuts and one it drops
    cut = dropped = 0
    for t in range(2 * LOADER_BATCHES):
        p = aug.params(0, t)
        ex = ds[int(order[t])]
        ex = hflip(ex) if p.flip else ex
        oh, ow, y0, x0, ch, cw = lsj_geometry(ex[0].shape[1], ex[0].shape[2], *p.lsj)
        for m in ex[3]:
            full = resize_nearest(np.asarray(m), (oh, ow))
            left, total = int(np.count_nonzero(full[y0:y0 + ch, x0:x0 + cw])), int(np.count_nonzero(full))
            cut += 0 < left < total
            dropped += left == 0
    assert cut >= 1 and dropped >= 1, (cut, dropped)
    _compare(ds, aug, max_gt)


@pytest.mark.parametrize('max_gt', [3, None])
def test_copy_paste_device_loader_equals_host_loader_on_a_multi_block_canvas(tmp_path, max_gt):
    ds, order = _dataset(tmp_path)
    aug = Augment(hflip_prob=0.5, seed=LOADER_SEED, lsj_size=LOADER_S, copy_paste_prob=1.0)
    # what the batches hold, by the host rule: a target instance that is cut, one covered entirely and dropped, and pasted instances
    tf = Transform(_Sizes())
    cut = dropped = pasted = 0
    for b in range(LOADER_BATCHES):
        exs = [tf(ds[int(order[2 * b + j])], aug.params(0, 2 * b + j)) for j in range(2)]
        plain = collate([e[:5] for e in exs], max_gt, canvas=LOADER_S)
        out = copy_paste_batch(plain, [e[5] for e in exs], [e[6] for e in exs], None)
        G = plain['labels'].shape[1]
        for n in range(2):
            assert exs[n][5] is True
            pick = np.zeros((G,), bool)
            offered = np.asarray(exs[1 - n][6], bool)[:G]
            pick[:len(offered)] = offered
            pick &= plain['labels'][1 - n] >= 0
            alpha = plain['masks'][1 - n, pick].any(0)
            left = [(int(np.count_nonzero(plain['masks'][n, g] * ~alpha)), int(np.count_nonzero(plain['masks'][n, g])))
                    for g in np.flatnonzero(plain['labels'][n] >= 0)]
            cut += sum(0 < l < t for l, t in left)
            dropped += sum(l == 0 for l, _ in left)
            pasted += int(pick.sum())
            assert int((out['labels'][n] >= 0).sum()) == sum(l > 0 for l, _ in left) + int(pick.sum())
    assert cut >= 1 and dropped >= 1 and pasted >= 1, (cut, dropped, pasted)
    _compare(ds, aug, max_gt)
