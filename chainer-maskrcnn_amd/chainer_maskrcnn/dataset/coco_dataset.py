"""COCO instance-mask and person-keypoint datasets for the host side of the training pipeline.

Role of chainer_maskrcnn/dataset/coco_dataset.py:11-161 in the reference (same class names, constructor arguments and
example tuples, so train.py's wiring is unchanged):

  COCOMaskLoader[i]      -> img (3,H,W) float32 RGB 0..255, bbox (G,4) float32 (y1,x1,y2,x2) built from the
                            integer-truncated COCO (x,y,w,h), label (G,) int32 = rank of the category among the selected
                            categories (COCO ids are not contiguous), masks = list of G (H,W) uint8 arrays
  COCOKeypointsLoader[i] -> img, bbox (G,4) with w,h >= 1, keypoints (G,17,3) (x,y,v)
  COCOKeypointsLoader.get_annotations(i) -> area, iscrowd, num_keypoints, raw bbox (x,y,w,h) of the same annotations (no image)
  COCOMaskLoader.get_annotations(i)      -> area, iscrowd, raw bbox (x,y,w,h), category id, image id (no image)
  COCOInstanceEvalDataset[i]             -> every image of the file (COCO box / mask AP): img, masks, labels, area, iscrowd, bbox, id

Built differently from the reference: the annotation file is indexed ONCE at construction into a per-image table
(boxes, labels and references to the segmentations), straight from ``coco_api.COCO``'s image->annotation index, so an
example costs a JPEG decode plus the mask rasterisation and no per-call annotation queries - the loader threads
(dataset/loader.py) call ``get_example`` concurrently.  No pycocotools, no chainercv: PIL decodes the image.
"""
import os

import numpy as np

from chainer_maskrcnn.dataset.coco_api import COCO

_SPLITS = {'train': 'train', 'val': 'val', 'validation': 'val'}


def read_image(path, color=True):
    """(C,H,W) float32, RGB order, values 0..255 (what chainercv.utils.read_image returns)."""
    from PIL import Image
    with Image.open(path) as f:
        img = np.asarray(f.convert('RGB' if color else 'P'), dtype=np.float32)
    return img[None] if img.ndim == 2 else np.ascontiguousarray(img.transpose(2, 0, 1))


def _yxyx(ann, min_side=0):
    x, y, w, h = (int(v) for v in ann['bbox'])
    if min_side:
        w, h = max(min_side, w), max(min_side, h)
    return (y, x, y + h, x + w)


class _CocoSplit(object):
    """One annotation file + image directory; ``records`` = [(file name, image id, annotations kept)]."""

    def __init__(self, kind, anno_dir, img_dir, split, data_type):
        if split not in _SPLITS:
            raise ValueError('please pick split from \'train\', \'val\',\'validation\'')
        tag = _SPLITS[split] + data_type
        self.coco = COCO(os.path.join(anno_dir, '%s_%s.json' % (kind, tag)))
        self.img_dir = os.path.join(img_dir, tag)
        self.records = []

    def _index(self, keep):
        """keep(ann) -> bool.  Images (ascending id) with at least one kept annotation; annotation order = file order."""
        for img_id in sorted(self.coco.imgs):
            anns = [a for a in self.coco.imgToAnns.get(img_id, ()) if keep(a)]
            if anns:
                self.records.append((self.coco.imgs[img_id]['file_name'], img_id, anns))

    @property
    def img_infos(self):
        return [(name, img_id) for name, img_id, _ in self.records]

    @property
    def length(self):
        return len(self.records)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        return self.get_example(i)

    def _record(self, i):
        if not 0 <= i < len(self.records):
            raise IndexError('index is out of bounds.')
        name, _, anns = self.records[i]
        return read_image(os.path.join(self.img_dir, name), color=True), anns


class COCOMaskLoader(_CocoSplit):
    def __init__(self, anno_dir='data/annotations', img_dir='data', split='train', data_type='2014', category_filter=None):
        super().__init__('instances', anno_dir, img_dir, split, data_type)
        self.cat_ids = self.coco.getCatIds(catNms=list(category_filter or []))
        self._label_of = {c: k for k, c in enumerate(self.cat_ids)}
        self._index(lambda a: a['category_id'] in self._label_of)
        # box / label arrays are fixed per image: computed here, not per example
        self._boxes = [np.array([_yxyx(a) for a in anns], np.float32).reshape(-1, 4) for _, _, anns in self.records]
        self._labels = [np.array([self._label_of[a['category_id']] for a in anns], np.int32) for _, _, anns in self.records]

    def get_example(self, i):
        img, anns = self._record(i)
        return img, self._boxes[i].copy(), self._labels[i].copy(), [self.coco.annToMask(a) for a in anns]

    def get_annotations(self, i):
        """The kept annotations of example i without reading the image (what COCO's box and mask AP need): {'area': (G,) float64,
        'iscrowd': (G,) bool, 'bbox': (G, 4) float64 raw (x, y, w, h), 'category_id': (G,) int64, 'image_id': int}."""
        if not 0 <= i < len(self.records):
            raise IndexError('index is out of bounds.')
        return _annotation_arrays(self.records[i][1], self.records[i][2])


def _annotation_arrays(img_id, anns):
    return {'area': np.array([a.get('area', 0.0) for a in anns], np.float64).reshape(-1),
            'iscrowd': np.array([bool(a.get('iscrowd', 0)) for a in anns], bool).reshape(-1),
            'bbox': np.array([a['bbox'] for a in anns], np.float64).reshape(-1, 4),
            'category_id': np.array([a['category_id'] for a in anns], np.int64).reshape(-1),
            'image_id': int(img_id)}


class COCOInstanceEvalDataset(object):
    """Every image of an instances annotation file, in ascending id (COCOeval's default imgIds), images without any kept annotation
    included - detections there are false positives in the official number.  Example i: (img (3,H,W) float32 0..255, gt_masks (G,H,W)
    uint8 (annToMask, crowd included), labels (G,) int32 (rank of the category among ``cat_ids``), area (G,) float64 (the annotations'
    own), iscrowd (G,) bool, bbox_xywh (G,4) float64 (raw), image_id).  With n, the first n images.  Categories as COCOMaskLoader."""

    def __init__(self, anno_dir='data/annotations', img_dir='data', split='val', data_type='2017', category_filter=None, n=None):
        split_ = _CocoSplit('instances', anno_dir, img_dir, split, data_type)
        self.coco, self.img_dir = split_.coco, split_.img_dir
        self.annotation_file = os.path.join(anno_dir, 'instances_%s%s.json' % (_SPLITS[split], data_type))
        self.cat_ids = self.coco.getCatIds(catNms=list(category_filter or []))
        self.label_names = [self.coco.cats[c]['name'] for c in self.cat_ids]
        self._label_of = {c: k for k, c in enumerate(self.cat_ids)}
        self.img_ids = sorted(self.coco.imgs)
        if n is not None:
            self.img_ids = self.img_ids[:n]

    def __len__(self):
        return len(self.img_ids)

    def get_annotations(self, i):
        if not 0 <= i < len(self.img_ids):
            raise IndexError('index is out of bounds.')
        img_id = self.img_ids[i]
        return _annotation_arrays(img_id, self._anns(img_id))

    def _anns(self, img_id):
        return [a for a in self.coco.imgToAnns.get(img_id, ()) if a['category_id'] in self._label_of]

    def __getitem__(self, i):
        if not 0 <= i < len(self.img_ids):
            raise IndexError('index is out of bounds.')
        img_id = self.img_ids[i]
        info = self.coco.imgs[img_id]
        anns = self._anns(img_id)
        img = read_image(os.path.join(self.img_dir, info['file_name']), color=True)
        h, w = info['height'], info['width']
        masks = np.array([self.coco.annToMask(a) for a in anns], np.uint8).reshape(len(anns), h, w)
        a = _annotation_arrays(img_id, anns)
        labels = np.array([self._label_of[c] for c in a['category_id']], np.int32).reshape(-1)
        return img, masks, labels, a['area'], a['iscrowd'], a['bbox'], img_id


class COCOKeypointsLoader(_CocoSplit):
    n_keypoints = 17

    def __init__(self, anno_dir='data/annotations', img_dir='data', split='train', data_type='2014'):
        super().__init__('person_keypoints', anno_dir, img_dir, split, data_type)
        person = set(self.coco.getImgIds(catIds=[1]))
        self._index(lambda a: a['image_id'] in person)       # every annotation of an image that shows a person
        self._boxes = [np.array([_yxyx(a, min_side=1) for a in anns], np.float32).reshape(-1, 4) for _, _, anns in self.records]
        self._kps = [np.array([a['keypoints'] for a in anns]).reshape(-1, self.n_keypoints, 3) for _, _, anns in self.records]

    def get_example(self, i):
        img, _ = self._record(i)
        return img, self._boxes[i].copy(), self._kps[i].copy()

    def get_annotations(self, i):
        """The kept annotations of example i without reading the image (what COCO's keypoint OKS and its ignore rule need):
        {'area': (G,) float64, 'iscrowd': (G,) bool, 'num_keypoints': (G,) int64, 'bbox': (G, 4) float64 raw (x, y, w, h)}."""
        if not 0 <= i < len(self.records):
            raise IndexError('index is out of bounds.')
        anns = self.records[i][2]
        return {'area': np.array([a.get('area', 0.0) for a in anns], np.float64).reshape(-1),
                'iscrowd': np.array([bool(a.get('iscrowd', 0)) for a in anns], bool).reshape(-1),
                'num_keypoints': np.array([a.get('num_keypoints', int(np.count_nonzero(np.asarray(a['keypoints'])[2::3] > 0)))
                                           for a in anns], np.int64).reshape(-1),
                'bbox': np.array([a['bbox'] for a in anns], np.float64).reshape(-1, 4)}
