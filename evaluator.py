"""The reference's evaluator.py (InstanceSegmentationVOCEvaluator, a copy of ChainerCV's) at the same place: re-exports the streaming
evaluators of chainer_maskrcnn/evaluator.py, which train.py --eval-interval attaches to the val split (KeypointCOCOEvaluator: COCO
keypoint AP of keypoint heads, --eval-metric keypoint_coco; InstanceSegmentationCOCOEvaluator: COCO mask and box AP, --eval-metric
mask_coco)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'chainer-maskrcnn_amd'))

from chainer_maskrcnn.evaluator import (InstanceSegmentationCOCOEvaluator, InstanceSegmentationVOCEvaluator,  # noqa: E402,F401
                                        KeypointCOCOEvaluator)
