"""COCO box and mask AP on the device: the run-length encoder (csrc/rle.hip through ops.mask_rle_encode) equals a NumPy encoder bit
for bit, InstanceSegmentationCOCOEvaluator equals both evaluate_coco_results on its own exported results and the CPU restatement of
COCOeval (test_coco_eval_cpu.py) on predict()'s outputs, train.py --eval-metric mask_coco logs its keys without perturbing training,
and evaluate.py writes its files."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from chainer_maskrcnn import evaluations  # noqa: E402
from chainer_maskrcnn._hip import ops  # noqa: E402
from chainer_maskrcnn.dataset import coco_api  # noqa: E402
from test_coco_eval_cpu import ref_cocoeval  # noqa: E402

DEV = 'cuda:0'


def np_rle(mask):
    """Reference encoder: Fortran flatten, positions where the value changes (the value before the first pixel is 0), differences."""
    flat = np.asarray(mask).flatten(order='F') != 0
    prev = np.concatenate(([False], flat[:-1]))
    q = np.flatnonzero(flat != prev)
    return np.diff(np.concatenate(([0], q, [flat.size]))).astype(np.int32)


def _patterned(rs, D, H, W):
    """D masks cycling through: all zero, all one, pixel (0,0), pixel (H-1,W-1), checkerboard (the most runs), random blobs, noise;
    set pixels carry random nonzero bytes."""
    m = np.zeros((D, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for d in range(D):
        k = d % 7
        if k == 1:
            m[d] = 1
        elif k == 2:
            m[d, 0, 0] = 1
        elif k == 3:
            m[d, H - 1, W - 1] = 1
        elif k == 4:
            m[d] = (yy + xx + d) & 1
        elif k == 5:
            for _ in range(rs.randint(1, 5)):
                y0, x0 = rs.randint(0, H), rs.randint(0, W)
                m[d, y0:y0 + rs.randint(1, H + 1), x0:x0 + rs.randint(1, W + 1)] = 1
        elif k == 6:
            m[d] = rs.rand(H, W) < 0.3
    return m * rs.randint(1, 256, size=m.shape).astype(np.uint8)


def _check(m_host, m_dev):
    offsets, counts, area = ops.mask_rle_encode(m_dev)
    assert offsets.dtype == counts.dtype == area.dtype == torch.int32 and offsets.is_cuda and counts.is_cuda
    D, H, W = m_host.shape
    want = [np_rle(m_host[d]) for d in range(D)]
    want_off = np.concatenate(([0], np.cumsum([len(w) for w in want]))).astype(np.int32)
    o, c, a = offsets.cpu().numpy(), counts.cpu().numpy(), area.cpu().numpy()
    np.testing.assert_array_equal(o, want_off)
    np.testing.assert_array_equal(c, np.concatenate(want) if D else np.zeros((0,), np.int32))
    np.testing.assert_array_equal(a, (m_host != 0).reshape(D, H * W).sum(1))
    for d in range(D):
        np.testing.assert_array_equal(coco_api.rle_decode(c[o[d]:o[d + 1]], H, W), m_host[d] != 0)
    again = ops.mask_rle_encode(m_dev)
    for x, y in zip((offsets, counts, area), again):
        assert torch.equal(x, y)
    return o, c


@pytest.mark.parametrize('H,W', [(1, 1), (1, 1025), (1025, 1), (3, 5), (375, 500), (480, 640), (1024, 1024)])
@pytest.mark.parametrize('D', [0, 1, 7, 100])
def test_rle_encode_equals_numpy(H, W, D):
    if D == 100 and H * W >= 480 * 640:
        D = 30                                          # host reference time; the 100-mask grid is covered at the smaller shapes
    rs = np.random.RandomState(H * 3 + W + D)
    m = _patterned(rs, D, H, W)
    _check(m, torch.from_numpy(m).to(DEV))


def test_rle_encode_views_at_byte_offsets_and_bool():
    rs = np.random.RandomState(7)
    D, H, W = 9, 37, 41
    m = _patterned(rs, D, H, W)
    for off in (1, 3, 8, 15):
        buf = torch.full((off + m.size + 32,), 255, dtype=torch.uint8, device=DEV)        # set bytes around the view must not count
        v = buf[off:off + m.size].view(m.shape)
        v.copy_(torch.from_numpy(m))
        _check(m, v)
    _check(m, torch.from_numpy(m != 0).to(DEV))


def test_rle_encode_masks_from_mask_paste():
    rs = np.random.RandomState(11)
    D, S, Cm, H, W = 40, 14, 81, 375, 500
    logits = torch.from_numpy(rs.standard_normal((D, S, S, Cm)).astype(np.float32) * 3).to(DEV)
    y0, x0 = rs.uniform(0, H - 20, D), rs.uniform(0, W - 20, D)
    bbox = np.stack([y0, x0, np.minimum(y0 + rs.uniform(5, 300, D), H), np.minimum(x0 + rs.uniform(5, 300, D), W)], 1).astype(np.float32)
    label = rs.randint(0, 80, D).astype(np.int32)
    pasted = ops.mask_paste(logits, torch.from_numpy(label).to(DEV), torch.from_numpy(bbox).to(DEV), (H, W))
    o, _ = _check(pasted.cpu().numpy(), pasted)
    assert o[-1] > 2 * D
    _check(pasted.cpu().numpy(), pasted.bool())


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------
def _coco_dir(tmp_path):
    """instances_val2017.json + PNGs: 80 categories (ids 1..80), polygons, uncompressed and compressed RLE, a crowd, and an image
    without annotations."""
    from PIL import Image
    rs = np.random.RandomState(3)
    (tmp_path / 'val2017').mkdir()
    images, anns = [], []
    for i, (h, w) in enumerate([(120, 150), (100, 130), (120, 150), (90, 120)]):
        img_id = 10 + 7 * i
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(tmp_path / 'val2017' / ('%d.png' % img_id))
        images.append({'id': img_id, 'file_name': '%d.png' % img_id, 'height': h, 'width': w})
        if i == 2:
            continue                                          # no annotation
        for j in range(4):
            x0, y0 = rs.uniform(0, w * .6), rs.uniform(0, h * .6)
            bw, bh = rs.uniform(10, w - x0), rs.uniform(10, h - y0)
            cat = int(rs.randint(1, 81))
            ann = {'id': len(anns) + 1, 'image_id': img_id, 'category_id': cat, 'iscrowd': 0, 'bbox': [x0, y0, bw, bh],
                   'area': float(bw * bh * rs.uniform(.5, 1.0))}
            if j == 0:
                ann['segmentation'] = [[x0, y0, x0 + bw, y0, x0 + bw * .5, y0 + bh]]
            else:
                m = np.zeros((h, w), np.uint8)
                m[int(y0):int(y0 + bh), int(x0):int(x0 + bw)] = 1
                counts = coco_api.rle_encode(m)
                ann['segmentation'] = {'size': [h, w], 'counts': counts.tolist() if j == 1 else coco_api.rle_to_string(counts)}
                ann['iscrowd'] = int(j == 3)
            anns.append(ann)
    cats = [{'id': c, 'name': 'c%d' % c} for c in range(1, 81)]
    with open(tmp_path / 'instances_val2017.json', 'w') as f:
        json.dump({'images': images, 'annotations': anns, 'categories': cats}, f)
    return str(tmp_path / 'instances_val2017.json')


def _reduced_model():
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=5, _test_shrink=dict(stages=(1, 1, 1, 1), width_div=2), min_size=160, max_size=260)
    m.use_preset('evaluate')
    m.score_thresh = 0.0125                         # random weights: ~uniform class probabilities (1/81 = 0.0123)
    return m


def _restatement(m, data):
    """The CPU literal COCOeval on predict()'s outputs: results in loadRes's form (segm area = pixel count, bbox area = w * h)."""
    segm, bbox = [], []
    for i in range(len(data)):
        img, gm, gl, ga, gc, gb, _ = data[i]
        masks, labels, scores = m.predict([torch.from_numpy(np.asarray(img, np.float32))])
        yx = m.last_bboxes[0].cpu().numpy().astype(np.float64)
        pm, pl, ps = masks[0].cpu().numpy(), labels[0].cpu().numpy(), scores[0].cpu().numpy()
        gts = [{'category_id': data.cat_ids[l], 'area': float(a), 'iscrowd': int(c), 'mask': gm[g], 'bbox': [float(v) for v in gb[g]]}
               for g, (l, a, c) in enumerate(zip(gl, ga, gc))]
        for t, out in (('segm', segm), ('bbox', bbox)):
            dts = []
            for d in range(len(pl)):
                box = [yx[d, 1], yx[d, 0], yx[d, 3] - yx[d, 1], yx[d, 2] - yx[d, 0]]
                dts.append({'category_id': data.cat_ids[pl[d]], 'score': float(ps[d]), 'mask': pm[d], 'bbox': box,
                            'area': float(np.count_nonzero(pm[d])) if t == 'segm' else box[2] * box[3]})
            out.append(([dict(g) for g in gts], dts))
    return ref_cocoeval(segm, 'segm'), ref_cocoeval(bbox, 'bbox')


def test_evaluator_equals_exported_results_and_the_cpu_restatement(tmp_path):
    from chainer_maskrcnn.dataset.coco_dataset import COCOInstanceEvalDataset
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, split_coco_results
    ann_file = _coco_dir(tmp_path)
    data = COCOInstanceEvalDataset(anno_dir=str(tmp_path), img_dir=str(tmp_path), split='val', data_type='2017')
    assert len(data) == 4 and data[2][1].shape[0] == 0
    m = _reduced_model()
    results = []
    ev = InstanceSegmentationCOCOEvaluator(data, m, label_names=data.label_names, results=results)
    rep = ev.evaluate()
    assert m.train is True and m.score_thresh == 0.0125                      # preset untouched, training state restored
    assert len(results) > 0 and {r['image_id'] for r in results} <= set(data.img_ids)
    segm, bbox = split_coco_results(results)
    for name, res in (('segm.json', segm), ('bbox.json', bbox)):
        with open(tmp_path / name, 'w') as f:
            json.dump(res, f)
    from_file = {t: evaluations.evaluate_coco_results(ann_file, str(tmp_path / ('%s.json' % t)), t) for t in ('segm', 'bbox')}
    want_segm, want_bbox = _restatement(m, data)
    for t, want in (('segm', want_segm), ('bbox', want_bbox)):
        assert set(ev.stats[t]) == set(want) and len(want) == 12
        assert ev.stats[t] == want, (t, ev.stats[t], want)
        assert from_file[t] == want, (t, from_file[t], want)
    assert rep['main/map'] == ev.stats['segm']['AP'] and rep['main/bbox/ar'] == ev.stats['bbox']['AR100']
    assert 'main/ap/c1' in rep and len([k for k in rep if k.startswith('main/ap/')]) == 80
    # COCO results format
    r0 = results[0]
    assert set(r0) == {'image_id', 'category_id', 'segmentation', 'bbox', 'score'} and isinstance(r0['score'], float)
    info = {i['id']: i for i in json.load(open(ann_file))['images']}
    assert r0['segmentation']['size'] == [info[r0['image_id']]['height'], info[r0['image_id']]['width']]


class _FixedBoxes(object):
    """A 'model' whose predict() returns the given (masks, labels, scores, boxes (y1,x1,y2,x2)) of each image in turn."""

    def __init__(self, preds):
        self.preds, self.i, self.train, self.device = preds, 0, True, torch.device(DEV)

    def predict(self, imgs):
        m, l, s, b = self.preds[self.i]
        self.i += 1
        self.last_bboxes = [torch.from_numpy(np.asarray(b, np.float32)).to(DEV)]
        return ([torch.from_numpy(m != 0).to(DEV)], [torch.from_numpy(np.asarray(l, np.int32)).to(DEV)],
                [torch.from_numpy(np.asarray(s, np.float32)).to(DEV)])


def test_ground_truth_as_predictions_gives_ap_one():
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, SyntheticCOCOEvalDataset
    from chainer_maskrcnn.utils.synthetic import make_batch
    data = SyntheticCOCOEvalDataset(4, 96, 128, n_fg_class=10, G=5)
    preds = []
    for i in range(len(data)):
        b = make_batch(data.first_seed + i, 1, 96, 128, G=5, n_fg_class=10)
        preds.append((data[i][1], data[i][2], np.linspace(1, 0.5, 5), b['bboxes'][0]))
    results = []
    r = InstanceSegmentationCOCOEvaluator(data, _FixedBoxes(preds), results=results).evaluate()
    for k in ('main/map', 'main/ap50', 'main/ap75', 'main/ar', 'main/bbox/map', 'main/bbox/ap50', 'main/bbox/ar'):
        assert r[k] == pytest.approx(1.0, abs=1e-12), (k, r[k])
    assert len(results) == 20


# ---- train.py --eval-metric mask_coco and evaluate.py ------------------------------------------------------------------------------------
def _args(out, extra):
    import train
    return train.build_parser().parse_args(['--out', out, '--iteration', '4', '--batch-size', '1', '--image-size', '256', '320',
                                            '--log-interval', '2', '--snapshot-interval', '4', '--label_file', '/nonexistent'] + extra)


def test_train_mask_coco_logs_keys_and_does_not_perturb_training(tmp_path):
    import train
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    train.run(_args(a, ['--eval-interval', '2', '--eval-images', '2', '--eval-metric', 'mask_coco']))
    train.run(_args(b, []))
    la = [json.loads(l) for l in open(os.path.join(a, 'log'))]
    lb = [json.loads(l) for l in open(os.path.join(b, 'log'))]
    assert [e['iteration'] for e in la] == [2, 4] == [e['iteration'] for e in lb]
    keys = ['validation/main/%s' % k for k in ('map', 'ap50', 'ap75', 'ap_small', 'ap_medium', 'ap_large', 'ar')]
    for e in la:
        for k in keys + [k.replace('main/', 'main/bbox/') for k in keys]:
            assert k in e and (e[k] == -1.0 or 0.0 <= e[k] <= 1.0), (k, e.get(k))
    assert not any(k.startswith('validation/') for e in lb for k in e)
    za, zb = np.load(os.path.join(a, 'model_4.npz')), np.load(os.path.join(b, 'model_4.npz'))
    assert sorted(za.files) == sorted(zb.files) and len(za.files) > 100
    for k in za.files:
        np.testing.assert_array_equal(za[k], zb[k], err_msg=k)
    for x, y in zip(la, lb):
        assert x['main/loss'] == y['main/loss']


def test_evaluate_script_end_to_end(tmp_path):
    import evaluate
    from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator
    _coco_dir(tmp_path)
    labels = tmp_path / 'labels.txt'
    labels.write_text('\n'.join('c%d' % c for c in range(1, 81)))
    out = tmp_path / 'out'
    argv = ['--synthetic', '0', '--anno-dir', str(tmp_path), '--img-dir', str(tmp_path), '--data-type', '2017', '--label_file',
            str(labels), '--score-thresh', '0.0125', '--out', str(out)]
    stats = evaluate.run(evaluate.build_parser().parse_args(argv))
    segm = json.load(open(out / 'segm_results.json'))
    bbox = json.load(open(out / 'bbox_results.json'))
    metrics = json.load(open(out / 'metrics.json'))
    assert len(segm) == len(bbox) > 0 and 'segmentation' in segm[0] and 'bbox' in bbox[0]
    assert metrics == stats and set(metrics) == {'segm', 'bbox'} and len(metrics['segm']) == 12
    args = evaluate.build_parser().parse_args(argv)
    m = evaluate.build_model(args)
    ev = InstanceSegmentationCOCOEvaluator(evaluate.build_dataset(args, 80), m)
    ev.evaluate()
    assert ev.stats == metrics
