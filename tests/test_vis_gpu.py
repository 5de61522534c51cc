"""GPU tests of the rendering of detections (csrc/vis.hip through chainer_maskrcnn._hip.ops.vis_render, chainer_maskrcnn/vis.py, demo.py):
every picture equals the NumPy restatement tests/vis_reference.py byte for byte - seeded random scenes over sizes, instance counts,
opacities, draw flags and primitive lists, the image rounding, painter's order, and end to end draw_instances / draw_keypoints on the
predictions of the reduced random-weight networks of test_tta_gpu.py, and demo.run in-process."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import vis_reference as ref  # noqa: E402
from chainer_maskrcnn import vis  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.model.maskrcnn import MaskRCNN  # noqa: E402

DEV = 'cuda:0'
F = np.float32
ALL = ops.VIS_DRAW_MASKS | ops.VIS_DRAW_CONTOURS | ops.VIS_DRAW_BOXES


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _eq(got, want):
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == want.shape, (got.shape, got.dtype, want.shape)
    want = torch.from_numpy(want)
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got != want).any(dim=2).nonzero()
        y, x = (int(v) for v in bad[0])
        raise AssertionError('%d pixels differ, the first at (y %d, x %d): got %s, want %s'
                             % (len(bad), y, x, got[y, x].tolist(), want[y, x].tolist()))


def _scene(seed, D, H, W, n_prims):
    """A seeded scene: a non-integral image that leaves 0..255 on both sides; overlapping masks (boxes and ellipses, several nonzero byte
    values) that touch every border, one all set and one all clear when D >= 3; boxes partly and wholly outside; a random drawing order;
    primitives of every kind, partly and wholly outside the image."""
    rs = np.random.RandomState(seed)
    img = rs.uniform(-30, 290, (3, H, W)).astype(F)
    masks = np.zeros((D, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    bbox = np.zeros((D, 4), F)
    for d in range(D):
        cy, cx = rs.uniform(-0.1 * H, 1.1 * H), rs.uniform(-0.1 * W, 1.1 * W)
        ry, rx = rs.uniform(2, 0.6 * H), rs.uniform(2, 0.6 * W)
        if d % 2:
            on = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        else:
            on = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)
        on &= rs.rand(H, W) < 0.97                                                        # holes: contours inside the shape
        masks[d] = np.where(on, rs.choice([1, 2, 128, 255]), 0)
        bbox[d] = [cy - ry + rs.uniform(-3, 3), cx - rx + rs.uniform(-3, 3), cy + ry + rs.uniform(-3, 3), cx + rx + rs.uniform(-3, 3)]
    if D >= 3:
        masks[1] = 255                                                                   # all set
        masks[2] = 0                                                                     # all clear
        bbox[1] = [0, 0, H - 1, W - 1]
        bbox[2] = [-1e9, np.nan, 1e9, np.inf]
    colors = rs.randint(0, 256, (D, 3)).astype(np.uint8)
    order = rs.permutation(D).astype(np.int32)
    rows = []
    for _ in range(n_prims):
        kind = rs.randint(0, 5)
        x0, y0 = rs.randint(-W // 2, W + W // 2), rs.randint(-H // 2, H + H // 2)
        x1, y1 = x0 + rs.randint(-W // 3, W // 3 + 1), y0 + rs.randint(-H // 3, H // 3 + 1)
        if kind in (ops.VIS_RECT, ops.VIS_FILL) and rs.rand() < 0.8:
            x1, y1 = max(x0, x1), max(y0, y1)
        p = {ops.VIS_RECT: rs.randint(1, 5), ops.VIS_SEGMENT: rs.randint(1, 8), ops.VIS_DISC: rs.randint(0, 12),
             ops.VIS_GLYPH: rs.randint(1, 5), ops.VIS_FILL: 0}[kind]
        if kind == ops.VIS_GLYPH:
            x1, y1 = rs.randint(0, len(vis.FONT) + 3), 0                                  # also indices past the font: a filled cell
        rows.append((kind, x0, y0, x1, y1, p, rs.randint(0, 1 << 24), rs.choice([0, 77, 128, 256, 256])))
    rows += [(ops.VIS_SEGMENT, -4096, -4096, 20479, 20479, 3, 0x00FF00, 256), (ops.VIS_DISC, -4000, 5, 0, 0, 4096, 0x0000FF, 128),
             (ops.VIS_FILL, 20000, 20000, 20479, 20479, 0, 0xFFFFFF, 256)][:min(n_prims, 3)]
    prims = np.array(rows, ops.VIS_PRIM).reshape(-1)
    return img, masks, bbox, colors, order, prims


def _both(img, masks, bbox, colors, order, a256, thickness, flags, prims, font=vis.FONT):
    got = ops.vis_render(_t(img), None if masks is None else _t(masks), None if bbox is None else _t(bbox), colors, order, a256, thickness,
                         flags, prims, font)
    want = ref.render(img, masks, bbox, colors, order, a256, thickness, flags, prims, font)
    _eq(got, want)
    return want


# ---- the renderer against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,H,W,n_prims', [(0, 37, 53, 12), (1, 37, 53, 0), (7, 37, 53, 40), (100, 37, 53, 300), (1, 240, 321, 40),
                                           (7, 240, 321, 300), (100, 240, 321, 24), (0, 480, 640, 24), (7, 480, 640, 24),
                                           (100, 480, 640, 8), (7, 9, 130, 24), (7, 131, 3, 24), (3, 1, 1, 5)])
def test_random_scenes_equal_the_restatement(D, H, W, n_prims):
    img, masks, bbox, colors, order, prims = _scene(1000 * D + H + W, D, H, W, n_prims)
    want = _both(img, masks, bbox, colors, order, 128, 2, ALL, prims)
    if D:
        assert (want != ref.round_image(img).astype(np.uint8)).any()                      # something was drawn
    if n_prims >= 300:
        assert len(prims) > 256                                                           # more than one LDS chunk of primitives


@pytest.mark.parametrize('alpha', [0.0, 0.5, 1.0])
@pytest.mark.parametrize('flags', range(8))
def test_every_flag_and_opacity(alpha, flags):
    img, masks, bbox, colors, order, prims = _scene(7, 7, 64, 75, 10)
    _both(img, masks, bbox, colors, order, vis.alpha_to_a256(alpha), 1 + flags % 3, flags, prims)
    if flags == 0:                                                                       # nothing of the instances is drawn
        _eq(ops.vis_render(_t(img), None, None, colors, order, 128, 1, 0, prims, vis.FONT), ref.render(img, prims=prims, font=vis.FONT))


def test_without_an_order_and_from_an_odd_address():
    img, masks, bbox, colors, _, prims = _scene(3, 5, 45, 67, 6)
    want = ref.render(img, masks, bbox, colors, None, 200, 3, ALL, prims, vis.FONT)
    for shift in (0, 1, 2, 3):                                                           # the mask buffer starts at any byte
        buf = torch.zeros((masks.size + 8,), dtype=torch.uint8, device=DEV)
        m = buf[shift:shift + masks.size].view(masks.shape)
        m.copy_(_t(masks))
        assert m.data_ptr() % 4 == (buf.data_ptr() + shift) % 4
        _eq(ops.vis_render(_t(img), m, _t(bbox), colors, None, 200, 3, ALL, prims, vis.FONT), want)
    _eq(ops.vis_render(_t(img), _t(masks != 0), _t(bbox), colors, None, 200, 3, ALL, prims, vis.FONT), want)      # bool masks
    again = ops.vis_render(_t(img), _t(masks), _t(bbox), colors, None, 200, 3, ALL, prims, vis.FONT)
    _eq(again, want)                                                                     # the same bytes on every run


def test_image_rounding():
    vals = np.array([-3.0, -0.5, -0.4, 0.49, 0.5, 1.5, 2.5, 127.5, 254.49, 254.5, 255.0, 255.4, 300.0, 1e30, -1e30, np.inf, -np.inf,
                     np.nan, 0.0], F)
    rs = np.random.RandomState(0)
    img = rs.choice(vals, (3, 21, 19)).astype(F)
    img[:, 0, :] = vals
    want = _both(img, None, None, None, None, 128, 1, 0, None, None)
    np.testing.assert_array_equal(want[0, :, 0], [0, 0, 0, 0, 1, 2, 3, 128, 254, 255, 255, 255, 255, 255, 0, 255, 0, 0, 0])
    frac = rs.uniform(-2, 258, (3, 33, 47)).astype(F)
    _both(frac, None, None, None, None, 128, 1, 0, None, None)


def test_painters_order():
    H, W = 12, 17
    img = np.zeros((3, H, W), F)
    masks = np.ones((2, H, W), np.uint8)
    bbox = np.array([[2, 3, 9, 13], [2, 3, 9, 13]], F)
    colors = np.array([[200, 0, 0], [0, 200, 0]], np.uint8)
    a = ops.vis_render(_t(img), _t(masks), _t(bbox), colors, [0, 1], 128, 1, ALL).cpu().numpy()
    b = ops.vis_render(_t(img), _t(masks), _t(bbox), colors, [1, 0], 128, 1, ALL).cpu().numpy()
    # inside: red then green at a = 128: (200 * 128 + 128) >> 8 = 100, then (100 * 128 + 128) >> 8 = 50 under the second colour's 100
    assert a[5, 8].tolist() == [50, 100, 0] and b[5, 8].tolist() == [100, 50, 0]
    assert a[0, 0].tolist() == [0, 200, 0] and b[0, 0].tolist() == [200, 0, 0]           # the image border is contour: the last one wins
    assert a[2, 5].tolist() == [0, 200, 0] and b[2, 5].tolist() == [200, 0, 0]           # the box outline: the last one wins
    np.testing.assert_array_equal(a, ref.render(img, masks, bbox, colors, [0, 1], 128, 1, ALL))
    np.testing.assert_array_equal(b, ref.render(img, masks, bbox, colors, [1, 0], 128, 1, ALL))
    assert (a != b).any()
    # primitives come after every instance, in array order
    prims = np.array([(ops.VIS_FILL, 0, 0, W, H, 0, 0x0000FF, 256), (ops.VIS_DISC, 8, 5, 0, 0, 2, 0xFF0000, 128)], ops.VIS_PRIM)
    c = ops.vis_render(_t(img), _t(masks), _t(bbox), colors, [0, 1], 128, 1, ALL, prims).cpu().numpy()
    assert c[0, 0].tolist() == [255, 0, 0] and c[5, 8].tolist() == [128, 0, 128]          # rgb = r | g << 8 | b << 16
    c2 = ops.vis_render(_t(img), _t(masks), _t(bbox), colors, [0, 1], 128, 1, ALL, prims[::-1].copy()).cpu().numpy()
    assert c2[5, 8].tolist() == [255, 0, 0]


def test_wrapper_refusals():
    img = torch.zeros((3, 8, 8), device=DEV)
    with pytest.raises(ValueError):
        ops.vis_render(img, torch.zeros((2, 8, 9), dtype=torch.uint8, device=DEV), None, np.zeros((2, 3), np.uint8), None, 128, 1, 1)
    with pytest.raises(ValueError):
        ops.vis_render(img, torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV), None, np.zeros((2, 3), np.uint8), [0, 2], 128, 1, 1)
    with pytest.raises(ValueError):
        ops.vis_render(img, None, None, np.zeros((2, 3), np.uint8), None, 128, 1, ops.VIS_DRAW_MASKS)
    with pytest.raises(ValueError):
        ops.vis_render(img, prims=np.array([(ops.VIS_DISC, 30000, 0, 0, 0, 1, 0, 256)], ops.VIS_PRIM))
    with pytest.raises(TypeError):
        ops.vis_render(img, torch.zeros((1, 8, 8), device=DEV), None, np.zeros((1, 3), np.uint8), None, 128, 1, 1)
    with pytest.raises(ValueError):
        ops.vis_render(torch.zeros((3, 1, ops.VIS_MAX_SIDE + 1), device=DEV))
    assert ops.vis_render(torch.zeros((3, 0, 5), device=DEV)).shape == (0, 5, 3)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def _mask_model():
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=5, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    # random weights: class probabilities close to uniform (1/81 = 0.0123), so the count falls steeply just above it: this image gives 2499
    # detections at 0.0125, 126 at 0.016 and 1 at 0.018
    m.score_thresh = 0.017
    return m


def _keypoint_model(K):
    m = MaskRCNN(n_fg_class=1, n_keypoints=K, head_arch='fpn_keypoint', n_mask_convs=2, device=DEV, seed=7,
                 _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.3
    return m


def _image():
    return torch.from_numpy((np.random.RandomState(0).rand(3, 120, 150) * 255).astype(F))


def _label_names():
    return open(os.path.join(ROOT, 'data', 'label_coco.txt')).read().strip().split('\n')


def _reference_instances(img, masks, bbox, labels, scores, names, alpha=0.5, color_by='class', thickness=2, flags=ALL, draw_labels=True):
    """The restatement fed the prediction's tensors copied to the host."""
    H, W = img.shape[1:]
    bbox_h, labels_h, scores_h = bbox.cpu().numpy(), labels.cpu().numpy(), scores.cpu().numpy()
    order, colors, prims = vis.instance_primitives(H, W, bbox_h, labels_h, scores_h, names, color_by, draw_labels, 1)
    np.testing.assert_array_equal(order, np.argsort(scores_h, kind='stable'))
    return ref.render(img.cpu().numpy(), masks.cpu().numpy(), bbox_h, colors, order, vis.alpha_to_a256(alpha), thickness, flags, prims,
                      vis.FONT)


def test_draw_instances_on_predictions():
    m = _mask_model()
    img = _image()
    names = _label_names()
    masks, labels, scores = m.predict([img])
    bbox = m.last_bboxes[0]
    D = int(labels[0].shape[0])
    assert 1 <= D <= 100
    x = img.to(DEV)
    want = _reference_instances(img, masks[0], bbox, labels[0], scores[0], names)
    _eq(vis.draw_instances(x, masks[0], bbox, labels[0], scores[0], label_names=names), want)
    assert (want != ref.round_image(img.numpy()).astype(np.uint8)).any()
    want = _reference_instances(img, masks[0], bbox, labels[0], scores[0], None, alpha=0.3, color_by='instance', thickness=1,
                                flags=ops.VIS_DRAW_MASKS | ops.VIS_DRAW_BOXES, draw_labels=False)
    _eq(vis.draw_instances(x, masks[0], bbox, labels[0], scores[0], alpha=0.3, color_by='instance', draw_contours=False, draw_labels=False,
                           thickness=1), want)
    m2, l2, s2 = m.predict([img])                                                        # drawing changed nothing of the prediction
    assert torch.equal(m2[0], masks[0]) and torch.equal(l2[0], labels[0]) and torch.equal(s2[0], scores[0])


@pytest.mark.parametrize('K', [17, 20])
def test_draw_keypoints_on_predictions(K):
    from chainer_maskrcnn.evaluator import SyntheticKeypointEvalDataset
    m = _keypoint_model(K)
    img = torch.from_numpy(SyntheticKeypointEvalDataset(1, 120, 150)[0][0])
    kps, labels, scores = m.predict_keypoints([img])
    bbox = m.last_bboxes[0]
    D = int(labels[0].shape[0])
    assert 1 <= D <= 100 and kps[0].shape == (D, K, 4)
    kp_h = kps[0].cpu().numpy()
    for on, thresh in (('prob', 0.0), ('logit', float(np.median(kp_h[:, :, 2])))):
        prims = vis.keypoint_primitives(kp_h, bbox.cpu().numpy(), scores[0].cpu().numpy(), kp_thresh=thresh, on=on, alpha=0.6)
        n_seg, n_disc = int((prims['kind'] == ops.VIS_SEGMENT).sum()), int((prims['kind'] == ops.VIS_DISC).sum())
        assert n_disc > 0 and (K == 17 or n_seg == 0)                                     # K != 17: dots only
        if on == 'prob':
            assert n_disc == D * K and n_seg == (D * 19 if K == 17 else 0)
        want = ref.render(img.numpy(), prims=prims, font=vis.FONT)
        _eq(vis.draw_keypoints(img.to(DEV), kps[0], bbox, scores[0], kp_thresh=thresh, on=on, alpha=0.6), want)
        assert (want != ref.round_image(img.numpy()).astype(np.uint8)).any()


# ---- demo.py ---------------------------------------------------------------------------------------------------------------------------------
def _demo_args(out, extra=()):
    import demo
    return demo.build_parser().parse_args(['--synthetic', '2', '--image-size', '96', '128', '--score-thresh', '0.017', '--json', '1',
                                           '--label_file', os.path.join(ROOT, 'data', 'label_coco.txt'), '--out', out] + list(extra))


@pytest.mark.parametrize('extra', [[], ['--tta-sizes', '128', '160', '--tta-hflip', '1', '--tta-max-size', '240', '--alpha', '0.25',
                                        '--color-by', 'instance', '--no-contours']])
def test_demo_run_in_process(tmp_path, monkeypatch, extra):
    import demo
    from PIL import Image
    from chainer_maskrcnn.dataset.coco_api import rle_from_string
    model = _mask_model()
    monkeypatch.setattr(demo, 'build_model', lambda args: model)                         # the reduced network instead of the flags' one
    out = str(tmp_path / 'demo')
    args = _demo_args(out, extra)
    written = demo.run(args)
    assert model.score_thresh == 0.017 and model.nms_thresh == 0.3
    stems = ['synthetic_0000', 'synthetic_0001']
    assert written == [os.path.join(out, s + e) for s in stems for e in ('.png', '.json')]
    names = _label_names()
    total = 0
    for stem, (_, img) in zip(stems, demo.images(args, [])):
        assert img.shape == (3, 96, 128) and img.dtype == F
        x = torch.from_numpy(img).to(DEV)
        masks, labels, scores = model.predict([x])                                       # the model keeps the run's test-time views
        bbox = model.last_bboxes[0]
        D = int(labels[0].shape[0])
        assert extra or D <= 100                                                         # (the test-time views find more)
        total += D
        pic = np.array(Image.open(os.path.join(out, stem + '.png')))
        assert pic.shape == (96, 128, 3) and pic.dtype == np.uint8
        kw = dict(alpha=0.25, color_by='instance', draw_contours=False) if extra else {}
        _eq(vis.draw_instances(x, masks[0], bbox, labels[0], scores[0], label_names=names, **kw), pic)
        flags = ALL & ~ops.VIS_DRAW_CONTOURS if extra else ALL
        want = _reference_instances(torch.from_numpy(img), masks[0], bbox, labels[0], scores[0], names, alpha=kw.get('alpha', 0.5),
                                    color_by=kw.get('color_by', 'class'), flags=flags)
        np.testing.assert_array_equal(pic, want)
        rec = json.load(open(os.path.join(out, stem + '.json')))
        assert (rec['height'], rec['width']) == (96, 128) and len(rec['detections']) == D
        lab, sc, bb = labels[0].cpu().numpy(), scores[0].cpu().numpy(), bbox.cpu().numpy()
        area = masks[0].reshape(D, -1).sum(dim=1).cpu().numpy()
        for d, det in enumerate(rec['detections']):
            assert det['category_id'] == int(lab[d]) and det['category_name'] == names[lab[d]] and det['score'] == float(sc[d])
            assert det['bbox'] == [float(bb[d, 1]), float(bb[d, 0]), float(bb[d, 3] - bb[d, 1]), float(bb[d, 2] - bb[d, 0])]
            assert det['segmentation']['size'] == [96, 128]
            runs = rle_from_string(det['segmentation']['counts'])
            assert int(runs[1::2].sum()) == int(area[d]) == det['area'] and int(runs.sum()) == 96 * 128
    assert total >= 1
    if extra:
        assert model.tta is not None
