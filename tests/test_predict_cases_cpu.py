"""Every case of tests/predict_cases.py sits on the edge it is named for, and the float32 NumPy oracle (oracle/predict.py) passes the judges
of tests/predict_judge.py against the float64 restatement (tests/predict_reference.py) - asserted from NumPy alone, on any machine.  A case
that misses its edge, or whose in-band pixel count breaks the paste condition, fails HERE instead of silently weakening the GPU comparison
in tests/test_predict_gpu.py / tests/test_keypoint_predict_gpu.py.  Run with -s to see the measured ratios predict_cases.py quotes."""
import numpy as np
import pytest

from oracle import predict as op
from tests import predict_cases as pc
from tests import predict_judge as pj
from tests import predict_reference as ref

F = np.float32


# ---- the restatement itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ssize,dsize', [(14, 1), (14, 5), (28, 28), (28, 57), (56, 300), (56, 7), (1, 3), (7, 97)])
def test_coefficients_are_the_oracles(ssize, dsize):
    """The float32 walk over cv2_linear_coef's taps and coefficients gives cv2_resize_linear_f32's bits: they are the oracle's."""
    m = np.random.RandomState(ssize * dsize).rand(ssize, ssize).astype(F)
    np.testing.assert_array_equal(ref._resize(m, dsize, dsize + 1, F).view(np.int32), op.cv2_resize_linear_f32(m, (dsize + 1, dsize)).view(np.int32))
    i0, i1, f = ref.cv2_linear_coef(ssize, dsize)
    assert f.dtype == F and (f >= 0).all() and (f < 1).all() and i0.min() >= 0 and i1.max() <= ssize - 1 and ((i1 - i0) <= 1).all()
    if ssize == dsize:
        assert (f == 0).all() and (i0 == np.arange(ssize)).all()               # the identity: every coefficient is 0


def test_reference_masks_are_paste_masks():
    """masks_from(paste_f32(...)) is oracle.predict.paste_masks bit for bit: the float32 values the band is measured with are the oracle's."""
    c = pc.paste_case('S28-c96')
    got = ref.masks_from(c['logit']['ref32'], c['size'])
    np.testing.assert_array_equal(got, op.paste_masks(c['logits'].transpose(0, 3, 1, 2), c['label'], c['bbox'], c['size']))
    assert got.any()


# ---- A: decode -----------------------------------------------------------------------------------------------------------------------
def test_decode_cases_cover_the_grid():
    cs = [pc.decode_case(n) for n in pc.DECODE_NAMES]
    assert {c['rois'].shape[0] for c in cs} == {1, 255, 256, 257}
    assert {(c['n_class'], c['box_out'].shape[1], c['loc0']) for c in cs} == {(81, 96, 88), (2, 8, 4), (21, 25, 21)}
    for lay in pc.DECODE_LAYOUTS:
        mine = [c for c in cs if c['n_class'] == lay[0]]
        assert {c['scale'] for c in mine} == set(pc.DECODE_SCALES) and {c['mean'] for c in mine} == {pc.MEAN0, pc.MEAN1}
        assert {c['rois'].shape[0] for c in mine} >= set(pc.DECODE_R)
    assert any(c['box_out'].shape[1] == c['loc0'] + 4 and c['loc0'] % 4 for c in cs)


@pytest.mark.parametrize('name', pc.DECODE_NAMES)
def test_decode_oracle_passes_the_judges(name):
    c = pc.decode_case(name)
    w = c['want']
    assert all(np.isfinite(v).all() for v in (c['rois'], c['box_out'], w['raw'], w['prob'], c['oracle_bbox'], c['oracle_prob']))
    rb, rp = pj.box_ratio(c['oracle_bbox'], w), pj.ratio(c['oracle_prob'], w['prob'])
    print('decode %-10s oracle box ratio %.3g (rtol %.3g), prob ratio %.3g (rtol %.3g)' % (name, rb, c['box_rtol'], rp, c['prob_rtol']))
    assert rb <= c['box_rtol'] and rp <= c['prob_rtol']
    assert 16 * pj.EPS32 <= c['box_rtol'] < 1e-4 and 16 * pj.EPS32 <= c['prob_rtol'] < 1e-4       # a tolerance, not a licence
    np.testing.assert_allclose(w['prob'].sum(1), 1.0, rtol=1e-12)
    assert (w['bbox'][:, 0::2] >= 0).all() and (w['bbox'][:, 0::2] <= c['size'][0]).all()
    assert (w['bbox'][:, 1::2] >= 0).all() and (w['bbox'][:, 1::2] <= c['size'][1]).all()


def test_decode_planted_rows_fire():
    c = pc.decode_case('planted')
    w, p, (H, W) = c['want'], c['planted'], c['size']
    raw, box = w['raw'], w['bbox']
    assert c['mean'] == pc.MEAN1 and {0, 255, 256} <= set(p.values())
    assert raw[p['top'], 0] < 0 < raw[p['top'], 2] < H and box[p['top'], 0] == 0
    assert raw[p['left'], 1] < 0 < raw[p['left'], 3] < W and box[p['left'], 1] == 0
    assert 0 < raw[p['bottom'], 0] < H < raw[p['bottom'], 2] and box[p['bottom'], 2] == H
    assert 0 < raw[p['right'], 1] < W < raw[p['right'], 3] and box[p['right'], 3] == W
    assert (raw[p['outside_high'], :2] > (H, W)).all() and (box[p['outside_high']] == (H, W, H, W)).all()
    assert (raw[p['outside_low'], 2:] < 0).all() and (box[p['outside_low']] == 0).all()
    r = c['rois']
    assert r[p['zero_height'], 0] == r[p['zero_height'], 2] and w['size'][p['zero_height'], 0] == 0 and w['size'][p['zero_height'], 1] > 0
    assert r[p['zero_width'], 1] == r[p['zero_width'], 3] and w['size'][p['zero_width'], 1] == 0 and w['size'][p['zero_width'], 0] > 0
    loc = c['box_out'][:, c['loc0'] + 2:c['loc0'] + 4].astype(np.float64) * np.asarray(c['std'][2:], F) + np.asarray(c['mean'][2:], F)
    np.testing.assert_allclose(loc[p['exp_plus4']], 4.0, atol=1e-5)
    np.testing.assert_allclose(loc[p['exp_minus4']], -4.0, atol=1e-5)
    assert (w['size'][p['exp_plus4']] > 500).all() and (w['size'][p['exp_minus4']] < 0.2).all()
    sat = w['prob'][p['saturated']]
    assert F(sat[17]) == 1 and (np.delete(sat, 17) < 1e-43).all() and (np.delete(sat, 17) > 0).all()       # 1, and float32 denormals
    o = c['oracle_prob'][p['saturated']]
    assert o[17] == 1 and (np.delete(o, 17) < pj.FLT_MIN).all()
    assert (w['prob'][p['equal']] == 1.0 / c['n_class']).all()


# ---- B: suppression ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', pc.NMS_NAMES + [pc.NMS_OVER_CAP])
def test_nms_case_shape(name):
    c = pc.nms_case(name)
    R, th = c['box'].shape[0], F(c['score_thresh'])
    assert c['n_class'] == 5 and c['l_begin'] == 1 and c['l_end'] in (4, 5) and sorted(c['want']) == list(range(1, c['l_end']))
    assert np.isfinite(c['box']).all() and (c['box'][:, 2] >= c['box'][:, 0]).all() and (c['box'][:, 3] >= c['box'][:, 1]).all()
    for l, keep in c['want'].items():
        n = int((c['prob'][:, l] > th).sum())
        assert len(keep) <= n and len(set(keep.tolist())) == len(keep) and (c['prob'][keep, l] > th).all()
        assert (np.diff(c['prob'][keep, l]) <= 0).all()                        # selection order: score descending
    if name.startswith('grid'):
        assert (c['prob'][:, [1, 4]] > th).all()                                   # n == R
        assert not (c['prob'][:, 3] > th).any() and len(c['want'][3]) == 0         # a class with no candidate
        if R >= 63:
            p2 = c['prob'][:, 2]
            assert (p2 == th).sum() == c['n_at'] == round(0.05 * R) and (p2 < th).sum() == c['n_at'] and (p2 > th).sum() == R - 2 * c['n_at']
            assert c['n_dup'] == round(0.1 * R)
            u, first, cnt = np.unique(c['box'], axis=0, return_index=True, return_counts=True)
            assert (cnt - 1).sum() == c['n_dup']                                     # exact duplicate boxes
            for l in (1, 2):
                _, tc = np.unique(c['prob'][:, l], return_counts=True)
                assert (tc > 1).sum() >= min(10, R // 8)                           # many tied scores
            assert 1 < len(c['want'][1]) < R                                       # it suppresses, and not everything


def test_nms_grid_reaches_every_loop_shape():
    g = {R: pc.class_nms_geometry(R) for R in pc.NMS_GRID_R}                       # class 1 and 4: n == R
    assert [g[R]['nw'] for R in (1, 63, 64, 65)] == [1, 1, 1, 2] and [g[R]['nw'] for R in (511, 512)] == [8, 8]
    assert [g[R]['trips'] for R in (255, 256, 257, 512)] == [1, 1, 2, 2]
    assert max(pc.NMS_GRID_R) == pc.CN_CAP and pc.nms_case(pc.NMS_OVER_CAP)['box'].shape[0] == pc.CN_CAP + 1


@pytest.mark.parametrize('l_end', [4, 5])
def test_nms_identical_boxes_keep_one(l_end):
    c = pc.nms_case('identical-e%d' % l_end)
    R = c['box'].shape[0]
    assert (c['box'] == c['box'][0]).all()
    assert c['want'][1].tolist() == [64] and (c['prob'][:, 1] == c['prob'][:, 1].max()).sum() == 3      # the highest index of the top score
    assert c['want'][2].tolist() == [R - 1] and c['want'][3].tolist() == [11]
    if l_end == 5:
        top = np.nonzero(c['prob'][:, 4] == c['prob'][:, 4].max())[0]
        assert len(top) > 1 and c['want'][4].tolist() == [top.max()]


@pytest.mark.parametrize('l_end', [4, 5])
def test_nms_disjoint_boxes_keep_all_in_order(l_end):
    c = pc.nms_case('disjoint-e%d' % l_end)
    R = c['box'].shape[0]
    assert R > 128 and max(float(pc.iou_f32(c['box'][i], c['box'][j])) for i in range(R) for j in range(i + 1, min(i + 18, R))) == 0
    for l, keep in c['want'].items():
        cand = np.nonzero(c['prob'][:, l] > F(c['score_thresh']))[0]
        order = cand[np.lexsort((-cand, -c['prob'][cand, l].astype(np.float64)))]      # score descending, then index descending
        np.testing.assert_array_equal(keep, order)
    assert len(c['want'][1]) == R and 0 < len(c['want'][2]) < R and len(c['want'][3]) == 0
    _, tc = np.unique(c['prob'][:, 1], return_counts=True)
    assert tc.max() >= 5


@pytest.mark.parametrize('l_end', [4, 5])
def test_nms_threshold_pairs(l_end):
    c = pc.nms_case('threshold-e%d' % l_end)
    b, t, T = c['box'], pc.THRESHOLD_BOXES, F(c['nms_thresh'])
    iou = lambda k: pc.iou_f32(b[t[k][0]], b[t[k][1]])
    assert iou('exact') == T and pc.iou_f32(b[1], b[0]) == T                       # exactly on it, in float32, either way round
    assert iou('below') < T and iou('above') > T
    assert T - iou('below') < 4 * pj.EPS32 and iou('above') - T < 4 * pj.EPS32     # beside it
    assert b[3, 3] == np.nextafter(b[1, 3], F(0)) and b[9, 3] == np.nextafter(b[1, 3], F(10))      # one ulp of one coordinate
    assert np.isnan(iou('zero_pair')) and pc.iou_f32(b[t['normal']], b[t['zero_inside']]) == 0
    assert c['want'][1].tolist() == [0, 2, 3, 4, 5, 6, 7, 8]                       # >= drops 1, keeps 3, drops 9; both zero boxes stay
    assert c['want'][2].tolist() == [9, 7, 6, 5, 4, 3, 2, 1]
    assert c['want'][3].tolist() == [9, 7, 6, 5, 4, 3, 2, 1]                       # ties: index descending
    if l_end == 5:
        assert c['want'][4].tolist() == [8, 3, 2, 1, 7, 6, 5]                      # rows 4 and 9 sit on the score threshold


# ---- C: paste ------------------------------------------------------------------------------------------------------------------------
def test_paste_cases_cover_the_grid():
    cs = [pc.paste_case(n) for n in pc.PASTE_NAMES]
    assert {c['S'] for c in cs} == {14, 28, 56} and {c['Cm'] for c in cs} == {96, 4, 1}
    assert {c['size'] for c in cs} == {(1, 1), (1, 40), (40, 1), (97, 131), (513, 512)}
    assert any(len(c['bbox']) == 0 for c in cs)
    big = pc.paste_case('big-S56-c4')
    H, W = big['size']
    assert H * W > 262144 == pc.PASTE_GRID_PIXELS and len(big['bbox']) == 3
    wins = [r['win'] for r in big['logit']['ref64']]
    assert (7, 300) in [w[2:4] for w in wins] and (112, 113) in [w[2:4] for w in wins]
    assert any((w[0] + w[4]) * W > pc.PASTE_GRID_PIXELS and w[0] + w[4] == H and w[1] + w[5] == W for w in wins)      # pixels of the second trip
    for c in cs:
        assert ((c['label'] >= 0) & (c['label'] < c['Cm'])).all()
        if len(c['label']) >= 2:
            assert 0 in c['label'] and c['Cm'] - 1 in c['label']
        b = c['bbox']
        assert (b[:, :2] >= 0).all() and (b[:, 2] <= c['size'][0]).all() and (b[:, 3] <= c['size'][1]).all() and (b[:, 2:] >= b[:, :2]).all()


@pytest.mark.parametrize('name', ['S14-c4', 'S28-c96', 'S56-c1'])
def test_paste_standard_boxes(name):
    c = pc.paste_case(name)
    S, (H, W) = c['S'], c['size']
    dims = [r['win'][2:4] for r in c['logit']['ref64']]
    for must in [(1, 1), (5, 9), (S, S), (H, W), (6, 20)] + ([(2 * S, 2 * S + 1)] if S < 56 else []):
        assert must in dims, must
    assert any(mh == 0 and mw > 0 for mh, mw in dims) and any(mw == 0 and mh > 0 for mh, mw in dims)
    b = c['bbox'][dims.index((6, 20))]
    assert int(b[2]) - int(b[0]) == 7                                              # int(y2 - y1) != int(y2) - int(y1)
    assert any(r['win'][:2] == (H - 1, W - 1) and r['v'] is not None for r in c['logit']['ref64'])
    whole = c['logit']['ref64'][dims.index((H, W))]
    assert whole['win'] == (0, 0, H, W, H, W)


@pytest.mark.parametrize('entry', ['logit', 'prob'])
@pytest.mark.parametrize('name', pc.PASTE_NAMES)
def test_paste_condition_and_oracle(name, entry):
    """The condition of the paste judge, held by the reference alone: the pixels within the band of 128 are at most 1e-4 of the case's
    in-box pixels (at most 1 for the tiny boxes).  And the float32 oracle passes the judge."""
    c = pc.paste_case(name)
    e = c[entry]
    print('paste %-16s %-5s in-box %6d, oracle worst |v32 - v64| %.3g, band %.3g, in band %d' % (name, entry, e['n_in'], e['worst'], e['band'], e['n_band']))
    assert e['band'] >= pj.BAND_FLOOR and e['band'] < 1e-3 and e['worst'] < 1e-4
    assert e['n_band'] <= max(1, 1e-4 * e['n_in'])
    oracle = ref.masks_from(e['ref32'], c['size'])
    assert pj.check_paste(oracle, e['ref64'], e['band']) == e['n_band']
    if len(c['bbox']):
        assert e['n_in'] > 0 and not oracle.all() and (oracle.any() or e['n_in'] < 10)
    if entry == 'logit':
        np.testing.assert_array_equal(oracle, op.paste_masks(c['logits'].transpose(0, 3, 1, 2), c['label'], c['bbox'], c['size']))


def test_paste_judge_catches_one_wrong_pixel():
    c = pc.paste_case('S14-c4')
    e = c['logit']
    good = ref.masks_from(e['ref64'], c['size'])
    pj.check_paste(good, e['ref64'], e['band'])
    i = [k for k, r in enumerate(e['ref64']) if r['win'][2:4] == (5, 9)][0]
    s, t, mh, mw, _, _ = e['ref64'][i]['win']
    for y, x in ((s + mh - 1, t + mw - 1), (s + mh, t), (s, t + mw)):              # the last pixel of a small box; one below; one to the right
        bad = good.copy()
        bad[i, y, x] ^= True
        with pytest.raises(AssertionError):
            pj.check_paste(bad, e['ref64'], e['band'])


# ---- D: keypoint decode --------------------------------------------------------------------------------------------------------------
def test_keypoint_shapes_reach_every_lane_split():
    geo = {s: pc.keypoint_geometry(s[3], s[0], s[1]) for s in pc.KEYPOINT_SHAPES}
    assert {g['P'] for g in geo.values()} == {1, 2, 8, 16, 64}
    for S in pc.KEYPOINT_S:
        assert {geo[s]['P'] for s in geo if s[0] == S} == {1, 2, 8, 16, 64}
    assert {g['nsplit'] for g in geo.values()} == {1, 3, 6, 12, 24, 49, 98, 392}
    assert geo[(14, 17, 32, 300)] == dict(P=8, nsplit=3) and (56, 256, 256, 3) not in geo and (56, 256, 256, 1) in geo
    assert len(geo) == 40


@pytest.mark.parametrize('shape', [(7, 4, 4, 3), (14, 5, 8, 1), (28, 17, 32, 3), (14, 33, 64, 1)])
def test_keypoint_case_has_its_ties(shape):
    c = pc.keypoint_case(*shape)
    S, K = c['S'], c['K']
    idx, y, x, logit, prob = c['want']
    h = c['heat'][..., :K].reshape(c['D'], S * S, K)
    assert (c['heat'][..., K:] == 1e4).all() and logit.max() < 1e3
    ties = (h == logit[:, None, :]).sum(1)
    assert (ties >= 2).mean() > 0.5                                                # the maximum more than once: the first one counts
    assert idx[0, 0] == 0 and ties[0, 0] == S * S and abs(prob[0, 0] * S * S - 1) < 1e-12
    assert (h[np.arange(c['D'])[:, None], idx, np.arange(K)[None, :]] == logit).all()
