"""A small COCO-format dataset written on the fly for the augmentation tests: lossless PNG images of odd and even widths, an instances
file (polygon masks, two categories) and a person-keypoints file (17 keypoints per person, some with v == 0)."""
import json
import os

import numpy as np

from chainer_maskrcnn.dataset.augment import COCO_KEYPOINT_NAMES


def write_coco(root, n_img=5, seed=0, keypoint_names=COCO_KEYPOINT_NAMES, sizes=None):
    """Writes root/annotations/{instances,person_keypoints}_train2017.json and root/train2017/<i>.png."""
    from PIL import Image
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'train2017'), exist_ok=True)
    rs = np.random.RandomState(seed)
    images, anns = [], []
    aid = 1
    for i in range(n_img):
        h, w = sizes[i] if sizes else (int(rs.randint(90, 130)), int(rs.randint(100, 160)))
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, 'train2017', '%d.png' % i))
        images.append({'id': i, 'file_name': '%d.png' % i, 'height': h, 'width': w})
        for _ in range(1 + i % 3):                       # ragged instance counts: 1, 2, 3, 1, ...
            bw, bh = int(rs.randint(20, 60)), int(rs.randint(20, 60))
            x, y = int(rs.randint(0, w - bw)), int(rs.randint(0, h - bh))
            poly = [x, y, x + bw, y + bh // 3, x + bw, y + bh, x + bw // 2, y + bh, x, y + bh // 2]
            kx, ky = rs.randint(x, x + bw, 17), rs.randint(y, y + bh, 17)
            v = rs.choice([0, 1, 2], 17)
            kp = np.stack([np.where(v > 0, kx, 0), np.where(v > 0, ky, 0), v], 1).reshape(-1)
            anns.append({'id': aid, 'image_id': i, 'category_id': int(rs.choice([1, 3])), 'bbox': [x, y, bw, bh], 'iscrowd': 0,
                         'area': float(bw * bh), 'segmentation': [poly], 'keypoints': [int(t) for t in kp],
                         'num_keypoints': int((v > 0).sum())})
            aid += 1
    cats = [{'id': 1, 'name': 'person', 'keypoints': list(keypoint_names)}, {'id': 3, 'name': 'car'}]
    json.dump({'images': images, 'annotations': anns, 'categories': cats},
              open(os.path.join(root, 'annotations', 'instances_train2017.json'), 'w'))
    person = [dict(a, category_id=1) for a in anns]
    json.dump({'images': images, 'annotations': person, 'categories': cats[:1]},
              open(os.path.join(root, 'annotations', 'person_keypoints_train2017.json'), 'w'))
    return root
