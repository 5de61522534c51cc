"""The Mask Scoring R-CNN kernels away from N = 2, G = 4, 28 x 28 logits and one grid pass (csrc/maskiou.hip),
through ops.* against tests/maskiou_reference.py on the cases of tests/maskiou_edge_cases.py (tests/test_maskiou_edge_cases_cpu.py holds
every case to its path without a device).

Yardsticks, as in tests/test_maskiou_gpu.py: the integer areas and counts equal the reference's; the target equals the float32
restatement bit for bit and float64 within 4.5 eps32 of the target; input assembly, its backward and the rescoring equal NumPy bit for
bit; the loss is judged as tests/loss_judge.py does; every kernel twice with the same bits.

What the older file cannot see, and a wrong variant each test rejects:
  513 masks                      `((int)blockIdx.x - Rm) * TB` of the summing workgroups - without the block offset area[512] is never written
  tiny masks                     `head = to16 < HW ? to16 : HW` and the `v0`, `v1` clamps of k_mask_area - a mask shorter than its head, chunks
                                 whose share is empty, a vector count that is no multiple of the 32 chunks
  narrow crops                   head / vector / tail of a line at every start residue; `y += TB / 16` past 32 lines
  small logit maps               `p < HWm` with HWm below and just above one trip of the workgroup
  Rm = 270000                    both grid-stride loops of k_maskiou_l2
  n_channels                     `ch < n_channels` in k_maskiou_target, k_maskiou_input_fwd, k_maskiou_l2 and k_maskiou_rescore: a label
                                 that selects a padding channel of the logits names no class (tested against the padded width, the row
                                 would read whatever the padding holds)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskiou_edge_cases as cases            # noqa: E402
import maskiou_reference as mr            # noqa: E402
from loss_judge import EPS32, ratio, rtol_from            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
I32 = torch.int32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _masks_at(masks, offset):
    """the masks on the device as a contiguous view that starts ``offset`` bytes behind a 16-byte boundary."""
    buf = torch.zeros((masks.size + 32,), dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + masks.size].view(masks.shape)
    view.copy_(_t(masks))
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view


def _target(c, offset=0):
    from chainer_maskrcnn._hip import ops
    a = (_masks_at(c['masks'], offset), _t(c['n_gt']), _t(c['sample_roi']), _t(c['gt_assign']), _t(c['label']), _t(c['n_pos']), c['n_sample'],
         c['rows'], _t(c['mask_out']), _t(c['gt_roi_mask']), c['n_fg'])
    outs = []
    for _ in range(2):
        o = ops.maskiou_target(*a, want_counts=True)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32), err_msg=k)
    return outs[0]


def _check_target(name, c, got):
    want = mr.target_counts(c)
    np.testing.assert_array_equal(got['area'], mr.mask_areas(c['masks'], c['n_gt']))
    np.testing.assert_array_equal(got['counts'], want)
    t32, t64 = mr.target_from_counts(want, np.float32), mr.target_from_counts(want, np.float64)
    np.testing.assert_array_equal(got['target'].view(np.uint32), t32.view(np.uint32))
    err = np.abs(got['target'].astype(np.float64) - t64)
    print('%s: target max err %.2f eps32 of the target, %d rows > 0' % (name, float((err / np.maximum(t64, 1e-300)).max() / EPS32), int((t64 > 0).sum())))
    assert (err <= 4.5 * EPS32 * t64).all()


@pytest.mark.parametrize('case', cases.AREA_CASES, ids=cases.AREA_IDS)
def test_areas_of_tiny_and_of_many_masks(case):
    c = cases.area_case(*case)
    got = _target(c, offset=case[4])
    _check_target(cases.AREA_IDS[cases.AREA_CASES.index(case)], c, got)
    assert got['area'][-1, -1] > 0 and not got['area'][0].any()
    clean = dict(c, masks=c['masks'].copy())
    for i in range(case[0]):
        clean['masks'][i, c['n_gt'][i]:] = 0                            # the junk of the unused slots does not matter
    np.testing.assert_array_equal(_target(clean, offset=case[4])['area'], got['area'])


@pytest.mark.parametrize('mask_size', cases.MASK_SIZES)
def test_target_on_narrow_crops_and_small_logit_maps(mask_size):
    c = cases.crop_case(mask_size)
    got = _target(c)
    _check_target('mask_size %d' % mask_size, c, got)
    rows = c['rows']
    assert (got['target'] > 0).any() and not got['counts'][cases.PAD_ROW::rows].any() and not got['target'][cases.PAD_ROW::rows].any()
    assert not got['counts'][16::rows].any()


@pytest.mark.parametrize('C', cases.INPUT_C)
@pytest.mark.parametrize('P', cases.INPUT_P)
def test_input_assembly_and_its_backward(P, C):
    from chainer_maskrcnn._hip import ops
    c = cases.input_case(P, C)
    a = (_t(c['feat']), _t(c['mask_out']), _t(c['label']), cases.N_FG, c['cin_p'])
    got = ops.maskiou_input_fwd(*a)
    torch.cuda.synchronize()
    want = mr.input_fwd(c['feat'], c['mask_out'], c['label'], c['cin_p'], n_channels=cases.N_FG)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert got.shape == (6, P, P, C + 4) and not want[4, :, :, C].any() and want[1, :, :, C].all()
    assert torch.equal(ops.maskiou_input_fwd(*a).view(I32), got.view(I32))
    outs = []
    for _ in range(2):
        buf = torch.full((c['g_pool'].size + 1024,), 7.0, device=DEV)
        view = buf[:c['g_pool'].size].view(c['g_pool'].shape)
        view.copy_(_t(c['g_pool']))
        out = ops.maskiou_input_bwd(_t(c['g_in']), view)
        torch.cuda.synchronize()
        assert out.data_ptr() == view.data_ptr() and bool((buf[c['g_pool'].size:] == 7.0).all())
        outs.append(view.cpu().numpy())
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    np.testing.assert_array_equal(outs[0].view(np.uint32), mr.input_bwd(c['g_in'], c['g_pool']).view(np.uint32))


def test_l2_loss_past_one_grid_pass():
    from chainer_maskrcnn._hip import ops
    c = cases.l2_case()
    weight = 1.5
    a = (_t(c['pred']), _t(c['target']), _t(c['label']), cases.N_FG)
    out_t, gx_t = ops.maskiou_l2(*a, weight=weight)
    torch.cuda.synchronize()
    out, gx = out_t.cpu().numpy(), gx_t.cpu().numpy()
    w_loss, w_count, w_gx = mr.l2(c['pred'], c['target'], c['label'], weight, dtype=np.float64, n_channels=cases.N_FG)
    f_loss, _, f_gx = mr.l2(c['pred'], c['target'], c['label'], weight, dtype=np.float32, n_channels=cases.N_FG)
    rl, rg = rtol_from(np.array([f_loss]), np.array([w_loss])), rtol_from(f_gx, w_gx)
    print('l2 Rm %d: loss %.1f eps32 (bar %.1f), gradient %.1f eps32 (bar %.1f)' % (cases.L2_ROWS, ratio(out[:1], [w_loss]) / EPS32, rl / EPS32,
                                                                                    ratio(gx, w_gx) / EPS32, rg / EPS32))
    assert out[1] == w_count
    assert ratio(out[:1], np.array([w_loss])) <= rl and ratio(gx, w_gx) <= rg
    assert not gx[w_gx == 0].any() and gx[w_gx != 0].all()
    assert gx[-1, cases.N_FG - 1] != 0 and not gx[c['label'] == cases.N_FG + 1].any()       # the last row counts; a padding column never does
    out2, gx2 = ops.maskiou_l2(*a, weight=weight)
    assert torch.equal(out2.view(I32), out_t.view(I32)) and torch.equal(gx2.view(I32), gx_t.view(I32))


def test_rescore_past_one_workgroup():
    from chainer_maskrcnn._hip import ops
    c = cases.rescore_case()
    a = (_t(c['score']), _t(c['pred']), _t(c['label']), cases.RESCORE_CH)
    got = ops.maskiou_rescore(*a)
    torch.cuda.synchronize()
    want = mr.rescore(c['score'], c['pred'], c['label'], cases.RESCORE_CH)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert not want[:4].any() and want[-1] > 0 and want[4:].any()
    assert torch.equal(ops.maskiou_rescore(*a).view(I32), got.view(I32))
