"""GPU parity tests: device proposal path (rpn.hip) against the NumPy oracle (oracle/boxes.py,
oracle/proposal.py).  Integer outputs (sort order, NMS keep lists, FPN levels) are bit-exact given
identical float inputs; decoded boxes involve exp() and are compared to 2 ulp-level tolerance, so
the end-to-end bit-exact case uses dh = dw = 0 (exp(0) == 1 on both sides)."""
import os

import numpy as np
import pytest
import torch

from oracle import boxes as ob
from oracle.proposal import ProposalCreator
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu

from chainer_maskrcnn._hip import ops  # noqa: E402

DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _rand_boxes(rs, n, size=400.0):
    c = rs.uniform(0, size, (n, 2))
    hw = np.exp(rs.uniform(np.log(8), np.log(200), (n, 2)))
    return np.concatenate([c - hw / 2, c + hw / 2], 1).astype(np.float32)


# 5000 / 12000 boxes = 79 / 188 chunks of 64: the reduction crosses several 48-chunk windows, with light (0.7) and heavy
# (0.3) suppression
@pytest.mark.parametrize('n,thresh', [(1, 0.7), (63, 0.7), (64, 0.5), (65, 0.3), (1000, 0.7), (5000, 0.7), (5000, 0.3), (12000, 0.5)])
def test_nms_keep_list_bit_exact(n, thresh):
    rs = np.random.RandomState(n)
    b = _rand_boxes(rs, n)
    if n > 100:      # duplicates and threshold-equal pairs
        b[10] = b[3]
        b[11] = [0, 0, 10, 10]
        b[12] = [0, 0, 10, 7]        # IoU exactly 0.7 with box 11
    want = ob.nms(b, thresh)
    keep, nk = ops.nms(torch.from_numpy(b).to(DEV), thresh)
    nk = int(nk.item())
    assert nk == len(want)
    np.testing.assert_array_equal(keep.cpu().numpy()[:nk], want)


# The walk works in super-chunks of 256 boxes inside windows of 48 chunks (3072 boxes): sizes on and around those
# boundaries, the largest supported input, sparse boxes (almost nothing suppressed: every chunk keeps 64) and dense ones, and
# max_keep values that stop the walk inside a chunk, at a chunk end and at a super-chunk end.
@pytest.mark.parametrize('n,spread,thresh,max_keep', [(255, 400, 0.5, None), (256, 400, 0.5, None), (257, 400, 0.5, None),
                                                      (3071, 3000, 0.7, None), (3072, 3000, 0.7, None), (3073, 3000, 0.7, None),
                                                      (6200, 20000, 0.7, None), (16384, 4000, 0.6, None), (16384, 60000, 0.7, 2000),
                                                      (9000, 2000, 0.7, 1), (9000, 2000, 0.7, 64), (9000, 2000, 0.7, 65),
                                                      (9000, 2000, 0.7, 256), (9000, 2000, 0.7, 300)])
def test_nms_walk_boundaries(n, spread, thresh, max_keep):
    rs = np.random.RandomState(n + (max_keep or 0))
    b = _rand_boxes(rs, n, float(spread))
    want = ob.nms(b, thresh)
    if max_keep:
        want = want[:max_keep]
    keep, nk = ops.nms(torch.from_numpy(b).to(DEV), thresh, max_keep=max_keep)
    nk = int(nk.item())
    assert nk == len(want)
    np.testing.assert_array_equal(keep.cpu().numpy()[:nk], want)


def test_nms_max_keep_and_empty():
    rs = np.random.RandomState(2)
    b = _rand_boxes(rs, 500)
    want = ob.nms(b, 0.7)[:50]
    keep, nk = ops.nms(torch.from_numpy(b).to(DEV), 0.7, max_keep=50)
    assert int(nk.item()) == 50
    np.testing.assert_array_equal(keep.cpu().numpy(), want)
    keep, nk = ops.nms(torch.zeros((0, 4), device=DEV), 0.7)
    assert int(nk.item()) == 0


def test_fpn_levels_match_reference_golden():
    """tests/golden/levels_reference.npz was produced by the REFERENCE function
    (model/rpn/multilevel_region_proposal_network.py:16-31) in the build container."""
    z = np.load(os.path.join(GOLDEN, 'levels_reference.npz'))
    rois, want = z['rois'], z['levels']
    got = ops.map_rois_to_fpn_levels(torch.from_numpy(np.ascontiguousarray(rois, np.float32)).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(got, want.astype(np.float32))
    rs = np.random.RandomState(0)
    b = _rand_boxes(rs, 5000, 1000.0)
    np.testing.assert_array_equal(ops.map_rois_to_fpn_levels(torch.from_numpy(b).to(DEV)).cpu().numpy(),
                                  ob.map_rois_to_fpn_levels(b))


def _rpn_case(seed, N, feat_shapes, exact):
    rs = np.random.RandomState(seed)
    anchors = ob.fpn_anchors(feat_shapes)
    A = anchors.shape[0]
    locs = (rs.standard_normal((N, A, 4)) * 0.3).astype(np.float32)
    if exact:
        locs[:, :, 2:] = 0
    scores = rs.standard_normal((N, A, 2)).astype(np.float32)
    scores[:, 5:40, 1] = scores[0, 5, 1]          # tied scores: order must follow the (score desc, index desc) pin
    return anchors, locs, scores


# The top-n_pre selection is a radix select + an in-LDS bitonic sort whose shape depends on np, the power of two >= n_pre (n_pre clamped
# to A first).  Up to 2048 keys one workgroup sorts (k_sort_desc_lds<np>: 128 for n_pre = 100, 1024 for 600, 2048 for 2048); above that,
# runs of 2048 keys are sorted and merged by rank (k_merge_runs<np / 2048>: 2 for 2049 and 3000; 4 for the 12000 that this pyramid's
# A = 7,677 clamps; 8 - with the larger pyramid, A = 23,025 anchors - for the training size 12000 and for 16384).  Every other shape,
# unclamped n_pre of 4097..8192 among them, is in test_proposals_every_sort_shape below.
@pytest.mark.parametrize('n_pre,n_post,big', [(12000, 2000, False), (600, 100, False), (3000, 300, False), (100, 20, False),
                                              (12000, 2000, True), (2048, 300, False), (2049, 300, False), (16384, 2000, True)])
def test_proposals_end_to_end_bit_exact(n_pre, n_post, big):
    N = 2
    feat = [(72, 80), (36, 40), (18, 20), (9, 10), (5, 5)] if big else [(40, 48), (20, 24), (10, 12), (5, 6), (3, 3)]
    anchors, locs, scores = _rpn_case(1, N, feat, exact=True)
    img_size = (288, 320) if big else (160, 192)
    o = ops.rpn_proposals(torch.from_numpy(locs).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(anchors).to(DEV),
                          img_size, 16.0, n_pre, n_post, 0.7, debug=True)
    pc = ProposalCreator(n_train_pre_nms=n_pre, n_train_post_nms=n_post)
    for i in range(N):
        want, dbg = pc(locs[i], scores[i, :, 1], anchors, img_size, return_debug=True)
        npre = int(o['n_pre'][i].item())
        assert npre == len(dbg['pre_nms_index'])
        np.testing.assert_array_equal(o['sorted_anchor'].cpu().numpy().reshape(N, -1)[i, :npre], dbg['pre_nms_index'])
        nk = int(o['n_rois'][i].item())
        assert nk == len(want)
        np.testing.assert_array_equal(o['keep'].cpu().numpy().reshape(N, -1)[i, :nk], dbg['nms_keep'])
        got = o['rois'].cpu().numpy().reshape(N, n_post, 4)[i]
        np.testing.assert_array_equal(got[:nk], want)
        assert np.all(got[nk:] == 0)
        idx = o['roi_indices'].cpu().numpy().reshape(N, n_post)[i]
        assert np.all(idx[:nk] == i) and np.all(idx[nk:] == -1)
        np.testing.assert_array_equal(o['levels'].cpu().numpy().reshape(N, n_post)[i, :nk], ob.map_rois_to_fpn_levels(want))


def test_proposals_per_image_size_and_scale_equal_separate_calls():
    """A padded batch of two images of different sizes / resize factors: with per_image (h, w, min_size * scale) every
    image's proposals are bitwise those of a batch-1 call with its own size - and they are checked against the oracle's
    ProposalCreator called the way the reference calls it (rpn/multilevel_region_proposal_network.py:156-164: that
    image's img_size and scale)."""
    N, n_pre, n_post = 2, 3000, 300
    feat = [(40, 48), (20, 24), (10, 12), (5, 6), (3, 3)]
    anchors, locs, scores = _rpn_case(4, N, feat, exact=True)
    sizes = np.array([[160, 192], [117, 150]], np.float32)
    scales = np.array([1.0, 1.75], np.float32)
    per = torch.from_numpy(np.concatenate([sizes, (16.0 * scales)[:, None]], 1).astype(np.float32)).to(DEV)
    dl, ds, da = (torch.from_numpy(v).to(DEV) for v in (locs, scores, anchors))
    o = ops.rpn_proposals(dl, ds, da, (160, 192), 16.0, n_pre, n_post, 0.7, per_image=per)
    for i in range(N):
        one = ops.rpn_proposals(dl[i:i + 1].contiguous(), ds[i:i + 1].contiguous(), da, tuple(sizes[i]), 16.0 * float(scales[i]), n_pre, n_post, 0.7)
        nk = int(one['n_rois'][0].item())
        assert nk == int(o['n_rois'][i].item())
        got = o['rois'].cpu().numpy().reshape(N, n_post, 4)[i]
        np.testing.assert_array_equal(got, one['rois'].cpu().numpy())
        want = ProposalCreator(n_train_pre_nms=n_pre, n_train_post_nms=n_post)(locs[i], scores[i, :, 1], anchors, tuple(sizes[i]), scale=float(scales[i]))
        np.testing.assert_array_equal(got[:nk], want)
        assert got[:nk, 2].max() <= sizes[i, 0] and got[:nk, 3].max() <= sizes[i, 1]
    assert not np.array_equal(o['rois'].cpu().numpy(), ops.rpn_proposals(dl, ds, da, (160, 192), 16.0, n_pre, n_post, 0.7)['rois'].cpu().numpy())


# ---- the selection / sort edges of tests/sampler_cases.py (each case's edge is asserted from the oracle in test_sampler_cases_cpu.py) ----
def _check_rpn_case(c):
    """n_pre, sorted_anchor, keep, rois, roi_indices and levels of every image against the oracle's, bit for bit."""
    N, n_eff, n_post = c['locs'].shape[0], c['n_eff'], c['n_post']
    per = None if c['per_image'] is None else torch.from_numpy(c['per_image']).to(DEV)
    o = ops.rpn_proposals(torch.from_numpy(c['locs']).to(DEV), torch.from_numpy(c['scores']).to(DEV), torch.from_numpy(c['anchors']).to(DEV),
                          c['img_size'], c['min_size'], c['n_pre'], n_post, 0.7, debug=True, per_image=per)
    o = {k: v.cpu().numpy() for k, v in o.items()}
    for i, w in enumerate(c['want']):
        npre = int(o['n_pre'][i])
        assert npre == len(w['pre_nms_index']), (i, npre, len(w['pre_nms_index']))
        np.testing.assert_array_equal(o['sorted_anchor'].reshape(N, n_eff)[i, :npre], w['pre_nms_index'], err_msg='image %d' % i)
        nk = int(o['n_rois'][i])
        assert nk == len(w['rois']), (i, nk, len(w['rois']))
        np.testing.assert_array_equal(o['keep'].reshape(N, n_post)[i, :nk], w['nms_keep'])
        got = o['rois'].reshape(N, n_post, 4)[i]
        np.testing.assert_array_equal(got[:nk], w['rois'])
        assert np.all(got[nk:] == 0)
        idx = o['roi_indices'].reshape(N, n_post)[i]
        assert np.all(idx[:nk] == i) and np.all(idx[nk:] == -1)
        np.testing.assert_array_equal(o['levels'].reshape(N, n_post)[i, :nk], w['levels'])
    return o


@pytest.mark.parametrize('n_pre', sc.SORT_SHAPES)
def test_proposals_every_sort_shape(n_pre):
    """np = 64 .. 2048 in one workgroup (k_sort_desc_lds<64>: n_pre 1, 63, 64; <256>: 256; <512>: 257, 512; <1024>: 513, 1024; <2048>: 1025),
    sorted runs + k_merge_runs<2> (4096), <4> (4097, 6000, 8192) and <8> (8193), n_pre on and beside every power of two."""
    _check_rpn_case(sc.rpn_sort_shape(n_pre))


@pytest.mark.parametrize('n_pre', [6000, 600])
def test_proposals_fewer_valid_boxes_than_n_pre_in_a_mixed_batch(n_pre):
    """Image 0 has more valid boxes than n_pre, image 1 fewer (1 .. 2047: the sort's and the merge's zero-padded tail, the n_valid rule of
    k_gather_sorted), image 2 none: n_pre = n_rois = 0, all rois 0, roi_indices -1."""
    c = sc.rpn_mixed_valid(n_pre)
    o = _check_rpn_case(c)
    assert o['n_pre'][2] == 0 and o['n_rois'][2] == 0
    assert not o['rois'].reshape(3, -1)[2].any() and np.all(o['roi_indices'].reshape(3, -1)[2] == -1)


def test_proposals_fewer_anchors_than_n_pre():
    """A = 75 < n_pre = 2000: the entry point clamps n_pre to A; the outputs are the oracle's with n_pre = 75."""
    _check_rpn_case(sc.rpn_fewer_anchors_than_n_pre())


def test_proposals_second_trip_of_the_compaction():
    """A = 524,288 + 2048 + 37: k_compact_ge's tile loop runs a second trip (256 workgroups x 2048 keys per trip); the 300 best scores sit
    on both sides of row 524,288, the last row among them."""
    _check_rpn_case(sc.rpn_second_compaction_trip())


@pytest.mark.parametrize('n_pre', [600, 6000])
@pytest.mark.parametrize('kind', ['equal', 'lowbit'])
def test_proposals_keys_that_differ_only_in_the_index(kind, n_pre):
    """Every score equal (positive in image 0, negative in image 1): the radix select walks through all 32 score bits into the index bits
    and the order is the index, descending.  'lowbit': three score values whose bit patterns are neighbours."""
    _check_rpn_case(sc.rpn_index_only_keys(kind, n_pre))


def test_proposals_special_scores():
    """+-inf, the largest and smallest normal, denormals of both signs and interleaved +0.0 / -0.0: the order is argsort_desc_pinned's, in
    which the two zeros are EQUAL and the index decides (k_decode adds +0.0 before orderable(), which would rank -0.0 below +0.0)."""
    _check_rpn_case(sc.rpn_special_scores())


@pytest.mark.parametrize('ci', [0, 1, 2, 3])
def test_proposals_equal_reference_golden(ci):
    """tests/golden/pc_reference.npz: RoIs produced by the REFERENCE's in-tree ProposalCreator (utils/proposal_creator.py)
    executed in the build container.  The device's decode -> clip -> filter -> select -> sort -> NMS chain must reproduce them
    bit for bit (dh = dw = 0 in these cases: no exp() rounding involved)."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pc_reference.npz'))
    g = lambda k: d['c%d_in_%s' % (ci, k)]
    loc, score, anchor = g('loc'), g('score'), g('anchor')
    A = anchor.shape[0]
    scores2 = np.stack([np.zeros(A, np.float32), score], 1)[None]
    n_pre, n_post = int(g('n_pre')), int(g('n_post'))
    o = ops.rpn_proposals(torch.from_numpy(loc[None]).to(DEV), torch.from_numpy(scores2).to(DEV), torch.from_numpy(anchor).to(DEV),
                          tuple(int(v) for v in g('img')), float(g('min_size')) * float(g('scale')), n_pre, n_post, 0.7)
    want = d['c%d_out_roi' % ci]
    nk = int(o['n_rois'][0].item())
    assert nk == len(want)
    np.testing.assert_array_equal(o['rois'].cpu().numpy()[:nk], want)
    np.testing.assert_array_equal(o['levels'].cpu().numpy()[:nk], ob.map_rois_to_fpn_levels(want))


def test_proposals_random_scales_decode_tolerance():
    """exp() differs by <= 2 ulp between NumPy and the device: boxes compared with tolerance."""
    N = 1
    feat = [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    anchors, locs, scores = _rpn_case(2, N, feat, exact=False)
    img_size = (128, 128)
    o = ops.rpn_proposals(torch.from_numpy(locs).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(anchors).to(DEV),
                          img_size, 16.0, 3000, 300, 0.7, debug=True)
    want, dbg = ProposalCreator(n_train_pre_nms=3000, n_train_post_nms=300)(locs[0], scores[0, :, 1], anchors, img_size,
                                                                            return_debug=True)
    nk = int(o['n_rois'][0].item())
    got = o['rois'].cpu().numpy()[:nk]
    m = min(nk, len(want), 50)          # the head of the list is stable under ulp-level box differences
    np.testing.assert_allclose(got[:m], want[:m], rtol=1e-5, atol=1e-4)
    assert abs(nk - len(want)) <= 3


def test_pack_unpack_roundtrip():
    rs = np.random.RandomState(5)
    N, H, W, Cp, A = 2, 5, 7, 32, 3
    head = rs.standard_normal((N, H, W, Cp)).astype(np.float32)
    Atot = H * W * A + 11
    locs = torch.zeros((N, Atot, 4), device=DEV)
    scores = torch.zeros((N, Atot, 2), device=DEV)
    ops.rpn_pack(torch.from_numpy(head).to(DEV), A, locs, scores, 11)
    # reference semantics: NCHW conv output -> transpose(0,2,3,1).reshape(n,-1,4)  (multilevel_rpn.py:133-141)
    want_l = head[..., :12].reshape(N, H * W * A, 4)
    want_s = head[..., 12:18].reshape(N, H * W * A, 2)
    np.testing.assert_array_equal(locs.cpu().numpy()[:, 11:], want_l)
    np.testing.assert_array_equal(scores.cpu().numpy()[:, 11:], want_s)
    gh = ops.rpn_unpack_grad(locs, scores, (N, H, W, Cp), A, 11).cpu().numpy()
    np.testing.assert_array_equal(gh[..., :18], head[..., :18])
    assert np.all(gh[..., 18:] == 0)


# ---- the one-launch pack / unpack of all pyramid levels (what the training step launches) and softmax2 -------------------------------
def _levels_reference(heads, A):
    """The NumPy statement of test_pack_unpack_roundtrip per level, concatenated over the levels (level order = anchor order)."""
    N = heads[0].shape[0]
    locs = np.concatenate([h[..., :4 * A].reshape(N, -1, 4) for h in heads], 1)
    scores = np.concatenate([h[..., 4 * A:6 * A].reshape(N, -1, 2) for h in heads], 1)
    return locs, scores


# L = 1, 5 and 8 (the most the launch takes) levels, a last level of one position, N = 1 and 2, channel counts that are padded
# (6A < Cp) and exactly full (Cp = 12 = 6A); the last case has N x positions x A = 1,053,366 items for the pack and N x positions x Cp / 2 =
# 3,511,220 for the unpack, both above the 4096 blocks x 256 threads of one pass of their launches: the grid-stride loops wrap
LEVEL_CASES = [(2, 3, 32, [(8, 10), (4, 5), (2, 3), (1, 2), (1, 1)]),
               (1, 3, 20, [(5, 7)]),
               (2, 2, 12, [(9, 7), (5, 4), (3, 3), (2, 2), (2, 1), (1, 3), (1, 2), (1, 1)]),
               (1, 1, 8, [(6, 5), (3, 3), (2, 1), (1, 1), (1, 1)]),
               (1, 1, 8, [(1, 1)]),
               (2, 3, 20, [(418, 420), (1, 1)])]


@pytest.mark.parametrize('N,A,Cp,shapes', LEVEL_CASES, ids=['N%d-A%d-Cp%d-L%d' % (n, a, c, len(s)) for n, a, c, s in LEVEL_CASES])
def test_pack_levels_and_unpack_grad_levels_bit_exact(N, A, Cp, shapes):
    import ctypes
    from chainer_maskrcnn._hip import check, lib, ptr, stream_ptr
    rs = np.random.RandomState(N + A + Cp + len(shapes))
    heads = [rs.standard_normal((N, h, w, Cp)).astype(np.float32) for h, w in shapes]
    L, offs = len(shapes), np.cumsum([0] + [h * w * A for h, w in shapes])
    Atot = int(offs[-1])
    want_l, want_s = _levels_reference(heads, A)
    hd = [torch.from_numpy(h).to(DEV) for h in heads]
    nan = float('nan')
    locs, scores = torch.full((N, Atot, 4), nan, device=DEV), torch.full((N, Atot, 2), nan, device=DEV)
    ops.rpn_pack_levels(hd, A, locs, scores)
    np.testing.assert_array_equal(locs.cpu().numpy(), want_l)
    np.testing.assert_array_equal(scores.cpu().numpy(), want_s)
    locs1, scores1 = torch.full((N, Atot, 4), nan, device=DEV), torch.full((N, Atot, 2), nan, device=DEV)
    for l in range(L):
        ops.rpn_pack(hd[l], A, locs1, scores1, int(offs[l]))
    assert torch.equal(locs1, locs) and torch.equal(scores1, scores)
    # the backward: gradients of locs / scores back into one NaN-filled head gradient per level; the padded channels 6A..Cp-1 come back zero
    glocs = rs.standard_normal((N, Atot, 4)).astype(np.float32)
    gscores = rs.standard_normal((N, Atot, 2)).astype(np.float32)
    gl, gs = torch.from_numpy(glocs).to(DEV), torch.from_numpy(gscores).to(DEV)
    gheads = [torch.full((N, h, w, Cp), nan, device=DEV) for h, w in shapes]
    ptrs = (ctypes.c_void_p * L)(*[g.data_ptr() for g in gheads])
    hws = (ctypes.c_int * L)(*[h * w for h, w in shapes])
    check(lib().mrcnn_rpn_unpack_grad_levels_f32(ptr(gl), ptr(gs), ptrs, hws, L, N, Cp, A, Atot, stream_ptr()))
    for l, (h, w) in enumerate(shapes):
        got = gheads[l].cpu().numpy()
        assert not np.isnan(got).any()
        np.testing.assert_array_equal(got[..., :4 * A], glocs[:, offs[l]:offs[l + 1]].reshape(N, h, w, 4 * A))
        np.testing.assert_array_equal(got[..., 4 * A:6 * A], gscores[:, offs[l]:offs[l + 1]].reshape(N, h, w, 2 * A))
        assert np.all(got[..., 6 * A:] == 0)
        assert torch.equal(ops.rpn_unpack_grad(gl, gs, (N, h, w, Cp), A, int(offs[l])), gheads[l])
    for g1, g2 in zip(ops.rpn_unpack_grad_levels(gl, gs, [(N, h, w, Cp) for h, w in shapes], A), gheads):
        assert torch.equal(g1, g2)
    # and the round trip: unpacking the packed values restores the heads' first 6A channels
    for l, g in enumerate(ops.rpn_unpack_grad_levels(locs, scores, [(N, h, w, Cp) for h, w in shapes], A)):
        np.testing.assert_array_equal(g.cpu().numpy()[..., :6 * A], heads[l][..., :6 * A])


def _softmax2_float32(x):
    """The kernel's arithmetic in NumPy float32 (the oracle whose own error sets rtol, tests/loss_judge.py)."""
    x = np.asarray(x, np.float32)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / (e[..., :1] + e[..., 1:])


@pytest.mark.parametrize('M', [1, 257, 2 * 23025])
def test_softmax2_float64(M):
    """(M,2) scores -> probabilities against float64 element by element (|got - want| <= rtol |want| + FLT_MIN, rtol = 4 x max(the float32
    NumPy arithmetic's own ratio, 4 eps32)); pairs a naive exp would overflow on, equal pairs, zeros; every pair sums to 1 within 2 eps32."""
    from tests import loss_reference as ref
    from tests.loss_judge import EPS32, ratio, rtol_from
    rs = np.random.RandomState(M)
    x = (rs.standard_normal((M, 2)) * 5).astype(np.float32)
    if M == 1:
        x[0] = [90, -90]
    else:
        x[:5] = [[90, -90], [-90, 90], [3.25, 3.25], [0, 0], [-77.5, -77.5]]
    got = ops.softmax2(torch.from_numpy(x).to(DEV)).cpu().numpy()
    want = ref.softmax2(x)
    rtol, r = rtol_from(_softmax2_float32(x), want), ratio(got, want)
    print('LOSSRATIO k_softmax2 %.2f eps32 (bound %.2f eps32)' % (r / EPS32, rtol / EPS32))
    assert r <= rtol, (r / EPS32, rtol / EPS32)
    assert np.all(np.abs(got.astype(np.float64).sum(-1) - 1.0) <= 2 * EPS32)
    if M > 1:
        np.testing.assert_array_equal(got[:5], np.array([[1, 0], [0, 1], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5]], np.float32))


def test_softmax2_foreground_probability_is_monotone_in_the_logit_difference():
    """The proposal sort orders by the foreground probability: across a sorted ramp of b - a it never decreases, whether a stays at 0 or
    the pair is (-d/2, d/2) (d a multiple of 1/8: every value and every difference is exact in float32)."""
    d = np.arange(-240, 241, dtype=np.float32) / 8
    x = np.concatenate([np.stack([np.zeros_like(d), d], 1), np.stack([-d / 2, d / 2], 1)])
    p = ops.softmax2(torch.from_numpy(x).to(DEV)).cpu().numpy()[:, 1].reshape(2, -1)
    assert np.all(np.diff(p, axis=1) >= 0) and p[0, 0] < 1e-12 and p[0, -1] == 1 and p[0, 240] == 0.5
    assert np.all(np.diff(p[:, 180:301], axis=1) > 0)              # |d| <= 7.5: neighbours 1/8 apart differ by far more than an ulp
