"""MaskRCNN model assembly on gfx950 kernels.

Mirror of chainer_maskrcnn/model/maskrcnn.py:23-155,261-276 (constructor :26-133, __call__ :135-155,
prepare :261-276) and of the ChainerCV ``FasterRCNN`` base-class attributes the train chain and
train.py rely on (loc_normalize_mean/std, use_preset, n_class).  Only the
combination the reference can actually train is backbone 'fpn' with head_arch 'fpn' or 'fpn_keypoint'
(README.md:39) - that is the hot path.  The legacy variants (backbone 'c4' / 'darknet', head_arch 'res5' / 'light';
SURVEY.md section 8 f-4) construct like in the reference and run forward through ``forward_legacy``.
``predict`` / ``_suppress`` are SURVEY.md section 8f "next" rows.
"""
import contextlib

import numpy as np
import torch

from chainer_maskrcnn.nn.core import ParamStore
from chainer_maskrcnn._hip import ops
from .extractor.feature_pyramid_network import DCN_STAGES, FeaturePyramidNetwork, dcn_stage_settings      # noqa: F401
from .rpn.multilevel_region_proposal_network import MultilevelRegionProposalNetwork
from .head.fpn_roi_mask_head import FPNRoIBoxHead, FPNRoIMaskHead, MaskIoUHead, PointHead

# Cascade R-CNN (Cai & Vasconcelos 2018): the stages' normalisation of the box deltas; stage 1's is the model's loc_normalize_std
CASCADE_STDS = ((0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1), (0.033, 0.033, 0.067, 0.067))


def cascade_settings(cascade_ious, cascade_stds=None, head_arch='fpn', backbone='fpn', pos_iou_thresh=0.5, stage1_std=CASCADE_STDS[0]):
    """The checked cascade arguments of MaskRCNN: None (off), or (ious, stds) - K = len(ious) IoU thresholds, 2 <= K <= 4, non-decreasing,
    the first the sampler's ``pos_iou_thresh``; K stds of 4 positive numbers, stage 1's being ``stage1_std``: ``cascade_stds`` (K entries whose
    first is ignored in favour of stage 1's own, or the K - 1 later ones) or, by default, CASCADE_STDS for K <= 3 and stage1_std / k for
    stage k otherwise.  ValueError for anything else, the legacy heads and backbones included."""
    if cascade_ious is None:
        if cascade_stds is not None:
            raise ValueError('cascade_stds without cascade_ious')
        return None
    if head_arch not in ('fpn', 'fpn_keypoint') or backbone != 'fpn':
        raise ValueError("cascade_ious exists for backbone 'fpn' with head_arch 'fpn' or 'fpn_keypoint', not %r / %r" % (backbone, head_arch))
    try:
        ious = tuple(float(v) for v in cascade_ious)
    except (TypeError, ValueError):
        raise ValueError('cascade_ious must be a sequence of numbers, got %r' % (cascade_ious,))
    K = len(ious)
    if not 2 <= K <= 4:
        raise ValueError('cascade_ious: %d stages, 2 to 4 expected' % K)
    if any(not 0 < v < 1 for v in ious) or any(b < a for a, b in zip(ious, ious[1:])):
        raise ValueError('cascade_ious must lie in (0, 1) and not decrease, got %r' % (ious,))
    if ious[0] != float(pos_iou_thresh):
        raise ValueError('cascade_ious[0] = %r is not the sampler\'s pos_iou_thresh %r' % (ious[0], pos_iou_thresh))
    s1 = tuple(float(v) for v in stage1_std)
    if cascade_stds is None:
        later = [CASCADE_STDS[k] if K <= 3 and s1 == CASCADE_STDS[0] else tuple(v / (k + 1) for v in s1) for k in range(1, K)]
    else:
        later = [tuple(float(v) for v in s) for s in cascade_stds]
        if len(later) == K:
            later = later[1:]
        if len(later) != K - 1:
            raise ValueError('cascade_stds: %d entries for %d stages' % (len(cascade_stds), K))
    stds = (s1,) + tuple(later)
    if any(len(s) != 4 or any(not (v > 0 and np.isfinite(v)) for v in s) for s in stds):
        raise ValueError('cascade_stds: every stage takes 4 positive numbers, got %r' % (stds,))
    return ious, stds


def mask_iou_setting(mask_iou, head_arch='fpn'):
    """The checked mask_iou argument of MaskRCNN as a bool; ValueError for a value that is no truth value and for the heads that have no
    binary mask to score (the keypoint head, the legacy 'res5' / 'light' heads)."""
    if mask_iou not in (False, True, 0, 1):
        raise ValueError('mask_iou must be True or False, got %r' % (mask_iou,))
    if mask_iou and head_arch != 'fpn':
        raise ValueError("mask_iou exists for head_arch 'fpn' only, not %r" % (head_arch,))
    return bool(mask_iou)


def point_rend_settings(point_rend=False, point_train_points=196, point_oversample=3, point_importance=0.75, subdivision_steps=2,
                        subdivision_points=784, head_arch='fpn', mask_iou=False):
    """The checked PointRend arguments of MaskRCNN: None when ``point_rend`` is off, else a dict with train_points P,
    oversample k, importance beta, n_candidates = k * P, n_important = floor(beta * P), subdivision_steps and subdivision_points.
    ValueError for a value out of range, for the heads that have no binary mask to refine (the keypoint head, the legacy 'res5' / 'light'
    heads) and together with ``mask_iou`` (the MaskIoU target is defined on the 28 x 28 mask)."""
    if point_rend not in (False, True, 0, 1):
        raise ValueError('point_rend must be True or False, got %r' % (point_rend,))
    if not point_rend:
        return None
    if head_arch != 'fpn':
        raise ValueError("point_rend exists for head_arch 'fpn' only, not %r (a keypoint head has no binary mask to refine)" % (head_arch,))
    if mask_iou:
        raise ValueError('point_rend together with mask_iou is not supported: the MaskIoU target is defined on the 28 x 28 mask')
    ints = dict(point_train_points=point_train_points, point_oversample=point_oversample, subdivision_steps=subdivision_steps,
                subdivision_points=subdivision_points)
    for k, v in ints.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('%s must be a positive integer, got %r' % (k, v))
    if isinstance(point_importance, bool) or not isinstance(point_importance, (int, float, np.integer, np.floating)) \
            or not 0.0 <= point_importance <= 1.0:
        raise ValueError('point_importance must be a number in [0, 1], got %r' % (point_importance,))
    P, k = int(point_train_points), int(point_oversample)
    if k * P > 4096:
        raise ValueError('point_oversample * point_train_points = %d candidates per row exceed the 4096 the selection kernel sorts' % (k * P))
    if int(subdivision_steps) > 2:      # 28 -> 56 -> 112: the grid one workgroup of the selection kernel holds
        raise ValueError('subdivision_steps must be at most 2 (a 112 x 112 grid), got %r' % (subdivision_steps,))
    return dict(train_points=P, oversample=k, importance=float(point_importance), n_candidates=k * P,
                n_important=int(np.floor(float(point_importance) * P)), subdivision_steps=int(subdivision_steps),
                subdivision_points=int(subdivision_points))


def dcn_settings(dcn_stages=None, dcn_modulated=False, backbone='fpn'):
    """The checked deformable-convolution arguments of MaskRCNN as (stages in network order - () when off, modulated):
    dcn_stage_settings' rule, and ValueError for another backbone than 'fpn'."""
    stages, modulated = dcn_stage_settings(dcn_stages, dcn_modulated)
    if stages and backbone != 'fpn':
        raise ValueError("dcn_stages exists for backbone 'fpn' only, not %r" % (backbone,))
    return stages, modulated


class MaskRCNN(object):
    feat_stride = 16
    # box post-processing of _suppress, off until use_soft_nms / use_box_voting / use_max_detections set them on an instance
    soft_nms = None                 # (method, sigma)
    vote_thresh = None
    max_detections = None
    # Cascade R-CNN box stages, off unless the constructor's cascade_ious sets them
    cascade = None                  # (ious, stds)
    cascade_heads = ()
    # Mask Scoring R-CNN, off unless the constructor's mask_iou builds the head
    maskiou_head = None
    mask_iou_rescore = True         # predict: score = box score x predicted mask IoU (False: the box score, on a model that has the head)
    last_box_scores = None          # predict: the box scores of the last call's detections, one array per image
    # PointRend, off unless the constructor's point_rend builds the head
    point_rend = None               # the settings dict of point_rend_settings
    point_head = None
    point_rend_refine = True        # predict: subdivide and refine the mask logits (False: paste the coarse 28 x 28 masks)
    last_point_grid = None          # predict: the refined (D,G,G) logit grid of the last image (None where nothing was refined)
    last_point_coarse = None        # ... and the coarse logits it started from

    def __init__(self, n_fg_class, n_keypoints=None, n_mask_convs=None, pretrained_model=None, min_size=600,
                 max_size=1000, ratios=[0.5, 1, 2], anchor_scales=[8], rpn_initialW=None, loc_initialW=None,
                 score_initialW=None, proposal_creator_params={}, backbone='fpn', head_arch='fpn',
                 device='cuda', seed=1234, _test_shrink=None, head_norm=None, gn_groups=32, cascade_ious=None, cascade_stds=None,
                 mask_iou=False, fpn_norm=None, point_rend=False, point_train_points=196, point_oversample=3, point_importance=0.75,
                 subdivision_steps=2, subdivision_points=784, dcn_stages=None, dcn_modulated=False):
        """dcn_stages: None = the reference's ResNet; a selection of 'res3', 'res4', 'res5' = every bottleneck of those stages runs its 3x3
        layer as a deformable convolution, modulated (v2) with ``dcn_modulated`` (the dconv_c3-c5 / mdconv_c3-c5
        configurations): ``<block>/conv2_offset/{W,b}`` directly behind ``<block>/conv2/W``, zero-initialised.  backbone 'fpn' only; mask and
        keypoint heads alike.  No accuracy effect has been measured.
        fpn_norm: None = the reference's pyramid; 'gn' = GroupNorm of ``gn_groups`` groups behind each of the eight FPN convolutions
        (DESIGN.md §3.23); backbone 'fpn' only.
        head_norm: None = the reference's heads; 'gn' = GroupNorm of ``gn_groups`` groups behind conv1 and every mask / keypoint
        convolution of the 'fpn' / 'fpn_keypoint' heads.
        cascade_ious: None = one box stage; (0.5, 0.6, 0.7) = Cascade R-CNN: K box stages trained at these IoU thresholds,
        stage k > 1 a box-only head ``head/cascade<k>/...`` registered directly behind the stage-1 head's parameters and fed stage k-1's
        refined boxes; ``cascade_stds`` their delta normalisation (cascade_settings).
        mask_iou: True = Mask Scoring R-CNN: a MaskIoU head ``head/maskiou/...`` behind every other head parameter (the
        cascade's included) regresses the IoU of each predicted mask; ``predict`` multiplies it into the score.  head_arch 'fpn' only.
        point_rend: True = PointRend: a point head ``head/point/...`` behind every other head parameter predicts the mask
        at single points from the stride-4 level and the coarse logits.  It trains on ``point_train_points`` points per mask row, the
        ``floor(point_importance * point_train_points)`` most uncertain of ``point_oversample`` times as many candidates and uniform ones;
        ``predict`` refines the 28 x 28 logits in ``subdivision_steps`` 2x steps, re-predicting the ``subdivision_points`` most uncertain
        cells of each.  head_arch 'fpn' only, not together with ``mask_iou``."""
        if n_fg_class is None:
            raise ValueError('The n_fg_class needs to be supplied as an argument')
        if head_norm not in (None, 'gn'):
            raise ValueError("head_norm must be None or 'gn', got %r" % (head_norm,))
        if head_norm is not None and head_arch in ('res5', 'light'):
            raise ValueError("head_norm=%r exists for head_arch 'fpn' and 'fpn_keypoint' only, not %r" % (head_norm, head_arch))
        if fpn_norm not in (None, 'gn'):
            raise ValueError("fpn_norm must be None or 'gn', got %r" % (fpn_norm,))
        if fpn_norm is not None and backbone != 'fpn':
            raise ValueError("fpn_norm=%r exists for backbone 'fpn' only, not %r" % (fpn_norm, backbone))
        self.head_norm, self.gn_groups, self.fpn_norm = head_norm, int(gn_groups), fpn_norm
        self.dcn_stages, self.dcn_modulated = dcn_settings(dcn_stages, dcn_modulated, backbone)
        self.cascade = cascade_settings(cascade_ious, cascade_stds, head_arch, backbone)
        self.mask_iou = mask_iou_setting(mask_iou, head_arch)
        self.point_rend = point_rend_settings(point_rend, point_train_points, point_oversample, point_importance, subdivision_steps,
                                              subdivision_points, head_arch, self.mask_iou)
        self.ps = ParamStore()
        shrink = _test_shrink or {}
        if backbone == 'fpn':
            self.extractor = FeaturePyramidNetwork(self.ps, fpn_norm=fpn_norm, gn_groups=self.gn_groups, dcn_stages=self.dcn_stages,
                                                   dcn_modulated=self.dcn_modulated, **shrink)
            self.rpn = MultilevelRegionProposalNetwork(
                anchor_scales=self.extractor.anchor_scales, feat_strides=self.extractor.feat_strides,
                in_channels=self.extractor.out_channels, mid_channels=self.extractor.out_channels,
                proposal_creator_params=proposal_creator_params, ps=self.ps)
        elif backbone == 'c4':          # legacy (maskrcnn.py:60-69): ResNet-50 C4 + ChainerCV's single-level RPN
            from .extractor.c4_backbone import C4Backbone
            from .rpn.region_proposal_network import RegionProposalNetwork
            self.extractor = C4Backbone(pretrained_model, ps=self.ps, **shrink)
            wd = shrink.get('width_div', 1)
            self.rpn = RegionProposalNetwork(1024 // wd, 516 // wd, ratios=ratios, anchor_scales=anchor_scales,
                                             feat_stride=self.feat_stride, initialW=rpn_initialW,
                                             proposal_creator_params=proposal_creator_params, ps=self.ps)
        elif backbone == 'darknet':     # legacy (maskrcnn.py:70-75)
            from .extractor.darknet import Darknet
            self.extractor = Darknet(ps=self.ps)
            self.rpn = MultilevelRegionProposalNetwork(
                anchor_scales=self.extractor.anchor_scales, feat_strides=self.extractor.feat_strides, in_channels=256,
                proposal_creator_params={'n_test_pre_nms': 50, 'n_test_post_nms': 10}, ps=self.ps)
        else:
            raise ValueError('unknown backbone: {}'.format(backbone))
        c = self.extractor.out_channels
        self.head_arch = head_arch
        if head_arch == 'res5':         # legacy (maskrcnn.py:81-89)
            from .head.resnet_roi_mask_head import ResnetRoIMaskHead
            self.head = ResnetRoIMaskHead(n_fg_class + 1, roi_size=7, spatial_scale=1. / self.feat_stride,
                                          loc_initialW=loc_initialW, score_initialW=score_initialW, mask_initialW=0.01,
                                          ps=self.ps, width_div=shrink.get('width_div', 1))
            self.predict_mask = True
        elif head_arch == 'light':      # legacy (maskrcnn.py:91-98)
            from .head.light_roi_mask_head import LightRoIMaskHead
            self.head = LightRoIMaskHead(n_fg_class + 1, roi_size=7, loc_initialW=loc_initialW, score_initialW=score_initialW,
                                         mask_initialW=0.01, ps=self.ps, in_channels=c)
            self.predict_mask = True
        elif head_arch == 'fpn':
            self.head = FPNRoIMaskHead(n_fg_class + 1, roi_size_box=7, roi_size_mask=14, loc_initialW=loc_initialW,
                                       score_initialW=score_initialW, mask_initialW=0.01, ps=self.ps, in_channels=c,
                                       fc_channels=1024 // shrink.get('width_div', 1), norm=head_norm, gn_groups=self.gn_groups)
            self.predict_mask = True
        elif head_arch == 'fpn_keypoint':
            if n_keypoints is None:
                raise ValueError('n_keypoints must be set in keypoint detection')
            from .head.fpn_roi_keypoint_head import FPNRoIKeypointHead
            self.head = FPNRoIKeypointHead(2, n_keypoints, roi_size_box=7, roi_size_mask=14,
                                           n_mask_convs=8 if n_mask_convs is None else n_mask_convs,
                                           loc_initialW=loc_initialW, score_initialW=score_initialW, mask_initialW=0.01,
                                           ps=self.ps, in_channels=c, fc_channels=1024 // shrink.get('width_div', 1), norm=head_norm,
                                           gn_groups=self.gn_groups)
            self.predict_mask = False
        else:
            raise ValueError('unknown head archtecture specified. {}'.format(head_arch))
        # Cascade R-CNN: the later box stages, behind every parameter of the stage-1 head (which keeps its names, shapes and offsets)
        self.cascade_heads = []
        if self.cascade is not None:
            for k in range(2, len(self.cascade[0]) + 1):
                self.cascade_heads.append(FPNRoIBoxHead(self.head.n_class, roi_size_box=7, loc_initialW=loc_initialW, score_initialW=score_initialW,
                                                        ps=self.ps, prefix='head/cascade%d' % k, in_channels=c,
                                                        fc_channels=1024 // shrink.get('width_div', 1), norm=head_norm, gn_groups=self.gn_groups))
        # Mask Scoring R-CNN: the MaskIoU head, behind every existing head parameter - each keeps its offset and its initial draw
        self.maskiou_head = None
        if self.mask_iou:
            self.maskiou_head = MaskIoUHead(self.head.n_class, ps=self.ps, prefix='head/maskiou', in_channels=c,
                                            fc_channels=1024 // shrink.get('width_div', 1))
            self.head.keep_mask_pool = True
        # PointRend: the point head, behind every other head parameter
        self.point_head = None
        if self.point_rend is not None:
            self.point_head = PointHead(self.head.n_class, ps=self.ps, prefix='head/point', in_channels=c,
                                        fc_channels=256 // shrink.get('width_div', 1))
        # FasterRCNN base-class state
        self.mean = np.array([122.7717, 115.9465, 102.9801], dtype=np.float32)[:, None, None]   # unused (maskrcnn.py:273-274)
        self.min_size, self.max_size = min_size, max_size
        self.loc_normalize_mean = (0., 0., 0., 0.)
        self.loc_normalize_std = (0.1, 0.1, 0.2, 0.2)
        self.use_preset('visualize')
        self.train = True
        self.tta = None                 # test-time augmentation, off (use_test_augmentation)
        self.device = torch.device(device)
        self.ps.materialise(self.device, seed)
        if self.cascade is not None:         # Detectron2's _ScaleGradient: every stage's pooled-feature gradient times the float32 1.0f / K
            inv_k = torch.from_numpy(np.array([np.float32(1.0) / np.float32(len(self.cascade[0]))], np.float32)).to(self.device)
            for h in self.box_stages:
                h.pool_grad_scale = inv_k
        self.freeze_state = (False, 0)

    def freeze(self, bn=False, at=0):
        """Fine-tuning recipe of the training step (off by default; inference is not affected).
        bn: every BatchNorm of the FPN's ResNet is frozen - the step computes it from avg_mean / avg_var with a constant gamma / beta
            (the bits of the inference layer), computes no gradient for them and updates neither them nor the running statistics.
        at = k in 0..5: the stem (conv1, bn1) and the stages res2 .. res{k} are not trained: no tape, no backward pass, parameters and
            momentum untouched by the optimizer (weight decay included).  k = 2 is the usual recipe; k = 5 trains FPN / RPN / heads only.
            Requires bn.
        ``freeze(False, 0)`` undoes it.  Call it before capturing a GraphedStep (an existing one re-captures by itself)."""
        if not hasattr(self.extractor, 'set_freeze'):
            if not bn and not at:
                return self
            raise ValueError('freeze() exists for the FPN ResNet backbone only')
        names = self.extractor.set_freeze(bn, at)
        self.ps.set_frozen(names)
        for n in names:                 # a frozen parameter's gradient slot is never written again: it carries zeros (all-reduce included)
            self.ps.g(n).zero_()
        self.freeze_state = (bool(bn), int(at))
        return self

    @property
    def n_class(self):
        return self.head.n_class

    @property
    def box_stages(self):
        """The box stages in order: the head, then the cascade's later stages."""
        return [self.head] + list(self.cascade_heads)

    @property
    def cascade_stds(self):
        """The delta normalisation of every box stage: stage 1's is loc_normalize_std."""
        return (tuple(self.loc_normalize_std),) + (tuple(self.cascade[1][1:]) if self.cascade is not None else ())

    def use_preset(self, preset):
        if preset == 'visualize':
            self.nms_thresh, self.score_thresh = 0.3, 0.7
        elif preset == 'evaluate':
            self.nms_thresh, self.score_thresh = 0.3, 0.05
        else:
            raise ValueError('preset must be visualize or evaluate')

    def use_test_augmentation(self, sizes, hflip=False, max_size=None, keypoint_flip_perm=None):
        """Test-time augmentation of ``predict`` / ``predict_keypoints`` (Detectron's TEST.BBOX_AUG / MASK_AUG / KPS_AUG; DESIGN.md
        §3.12): every image runs as the views (s, mirror=False) then, with hflip, (s, mirror=True) for each short side s of ``sizes``, the long
        side capped by ``max_size`` (default: the model's); the union of the views' box candidates is suppressed together, the mask
        probabilities and the keypoint heat maps (left / right channels swapped by ``keypoint_flip_perm`` in a mirrored view) are averaged
        over the views.  ``sizes=None`` turns it off (the initial state)."""
        if sizes is None:
            self.tta = None
            return
        if self.cascade is not None:
            raise ValueError('use_test_augmentation: test-time augmentation of a cascade model (cascade_ious) is not supported')
        if self.maskiou_head is not None:
            raise ValueError('use_test_augmentation: test-time augmentation of a Mask Scoring model (mask_iou) is not supported')
        if self.point_head is not None:
            raise ValueError('use_test_augmentation: test-time augmentation of a PointRend model (point_rend) is not supported')
        sizes = [int(s) for s in sizes]
        if not sizes or any(s <= 0 for s in sizes):
            raise ValueError('use_test_augmentation: sizes must be positive, got %r' % (sizes,))
        if len(set(sizes)) != len(sizes):
            raise ValueError('use_test_augmentation: duplicate sizes in %r' % (sizes,))
        if max_size is not None and int(max_size) <= 0:
            raise ValueError('use_test_augmentation: max_size must be positive, got %r' % (max_size,))
        n_views = len(sizes) * (2 if hflip else 1)
        if n_views > ops.TTA_VIEWS_MAX:
            raise ValueError('use_test_augmentation: %d views, at most %d' % (n_views, ops.TTA_VIEWS_MAX))
        perm = None
        if self.head_arch == 'fpn_keypoint':
            if hflip and keypoint_flip_perm is None:
                raise ValueError('use_test_augmentation: hflip on a keypoint model needs keypoint_flip_perm (coordinates are never mirrored '
                                 'without swapping the left / right channels)')
            if keypoint_flip_perm is not None:
                perm = [int(k) for k in keypoint_flip_perm]
                if sorted(perm) != list(range(self.head.n_keypoints)):
                    raise ValueError('use_test_augmentation: keypoint_flip_perm is not a permutation of the %d keypoints'
                                     % self.head.n_keypoints)
        self.tta = {'sizes': sizes, 'hflip': bool(hflip), 'max_size': None if max_size is None else int(max_size),
                    'keypoint_flip_perm': perm}

    def use_soft_nms(self, method, sigma=0.5):
        """Soft-NMS (Bodla et al. 2017; Detectron's TEST.SOFT_NMS) in place of the hard per-class NMS of ``predict`` /
        ``predict_keypoints``: a kept box lowers the scores of the remaining boxes of its class - 'linear': times 1 - IoU where IoU >=
        nms_thresh; 'gaussian': times exp(-IoU^2 / sigma) - and a box leaves when its score is no longer above score_thresh.  The
        returned scores are the decayed ones.  ``None`` turns it off (the initial state)."""
        if method is None:
            self.soft_nms = None
            return
        if method not in ('linear', 'gaussian'):
            raise ValueError("use_soft_nms: method must be None, 'linear' or 'gaussian', got %r" % (method,))
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.floating, np.integer)) or not float(sigma) > 0:
            raise ValueError('use_soft_nms: sigma must be positive, got %r' % (sigma,))
        self.soft_nms = (method, float(sigma))

    def use_box_voting(self, vote_thresh):
        """Box voting (Detectron's TEST.BBOX_VOTE, scoring method ID): the box of every kept detection becomes the
        score-weighted mean of the boxes of all candidates of its class (prob > score_thresh, before the NMS) whose IoU with it is >=
        ``vote_thresh`` (0 < vote_thresh <= 1; Detectron uses 0.8).  Scores do not change.  ``None`` turns it off (the initial state)."""
        if vote_thresh is None:
            self.vote_thresh = None
            return
        if isinstance(vote_thresh, bool) or not isinstance(vote_thresh, (int, float, np.floating, np.integer)) \
                or not 0 < float(vote_thresh) <= 1:
            raise ValueError('use_box_voting: vote_thresh must lie in (0, 1], got %r' % (vote_thresh,))
        self.vote_thresh = float(vote_thresh)

    def use_max_detections(self, n):
        """At most ``n`` detections per image (Detectron's TEST.DETECTIONS_PER_IM): the n highest scores over all classes, ties to the
        earlier row, kept in their order, before the mask / keypoint branch runs.  ``None`` turns it off (the initial state)."""
        if n is None:
            self.max_detections = None
            return
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError('use_max_detections: an integer >= 1 or None expected, got %r' % (n,))
        self.max_detections = int(n)

    def test_views(self, H, W):
        """The test-time views of an H x W image: [(oh, ow, mirror)] in view order (``prepare_size``'s rule with min_size = s)."""
        t = self.tta
        max_size = t['max_size'] or self.max_size
        views = []
        for s in t['sizes']:
            oh, ow = scaled_size(H, W, s, max_size)
            views.append((oh, ow, False))
            if t['hflip']:
                views.append((oh, ow, True))
        return views

    def to_nhwc4(self, x):
        """(N,3,H,W) float32 images on the device -> the extractor's (N,H,W,4) operand."""
        return ops.image_nchw3_to_nhwc4(x.contiguous())

    def forward_legacy(self, x, scale=1.):
        """The legacy wiring (backbone 'c4' / 'darknet' with head 'res5' / 'light'): extractor -> RPN -> head with the
        signature those heads have, ``head(h, rois, roi_indices, spatial_scale)``.  The reference's own ``__call__`` cannot
        drive them (it passes the FPN head's arguments, maskrcnn.py:148-154, and unpacks six RPN outputs where ChainerCV's
        RPN returns five) - upstream they were driven by the legacy MaskRCNNTrainChain, which is broken."""
        img_size = tuple(x.shape[2:])
        h = self.extractor(self.to_nhwc4(x))
        self.rpn.train = self.train
        out = self.rpn(h, img_size, scale)
        rpn_locs, rpn_scores, rois, roi_indices = out[:4]
        self.head.train = self.train
        scale_ = self.extractor.spatial_scales[0] if hasattr(self.extractor, 'spatial_scales') else 1. / self.feat_stride
        res = self.head(h, rois, roi_indices, scale_)
        return tuple(res) + (rois, roi_indices)

    def __call__(self, x, scale=1.):
        """Reference forward (:135-155).  x (N,3,H,W) on the device."""
        if self.head_arch in ('res5', 'light'):
            raise TypeError('MaskRCNN.__call__ passes the FPN head signature (maskrcnn.py:148-154), which the %r head does not '
                            'have - the reference fails here too; use forward_legacy()' % self.head_arch)
        img_size = tuple(x.shape[2:])
        h = self.extractor(self.to_nhwc4(x))
        self.rpn.train = self.train
        rpn_locs, rpn_scores, rois, roi_indices, anchor, levels = self.rpn(h, img_size, scale)
        levels = levels.clamp(0, len(h) - 1)
        indices_and_rois = torch.cat((roi_indices.to(torch.float32)[:, None], rois), dim=1)
        if self.train:
            roi_cls_locs, roi_scores, mask = self.head(h, indices_and_rois, levels, self.extractor.spatial_scales)
            return roi_cls_locs, roi_scores, rois, roi_indices, mask
        roi_cls_locs, roi_scores = self.head(h, indices_and_rois, levels, self.extractor.spatial_scales, train=False)
        return roi_cls_locs, roi_scores, rois, roi_indices, levels

    def prepare(self, img):
        """maskrcnn.py:261-276: resize so that the short side is min_size unless the long side would exceed max_size,
        then scale to [0,1] (no mean subtraction - SURVEY.md App. B-3).  img (3,H,W) float32 tensor with values 0..255
        on the device.  The resize is chainercv.transforms.resize = cv2.resize INTER_LINEAR on float32, here
        ``mrcnn_image_resize_f32`` (the same tap rule as the training Transform's device resize)."""
        _, H, W = img.shape
        oh, ow = self.prepare_size(H, W)
        return ops.image_resize_f32(img.to(self.device, torch.float32).contiguous(), oh, ow, 255.0)

    @contextlib.contextmanager
    def _inference_mode(self):
        """``self.train`` and ``core.TRAIN`` off for the block, restored after it."""
        from chainer_maskrcnn.nn import core
        keep_train, keep_core = self.train, core.TRAIN
        self.train, core.TRAIN = False, False
        try:
            yield
        finally:
            self.train, core.TRAIN = keep_train, keep_core

    def _xy5(self, box, scale=None):
        """Boxes (D,4) (y1,x1,y2,x2), times ``scale`` unless they are in the forward's frame already -> the branch's (D,5) RoIs
        (0, x1, y1, x2, y2)."""
        z = torch.zeros((box.shape[0], 1), device=self.device)
        xy = box[:, [1, 0, 3, 2]]
        return torch.cat((z, xy if scale is None else xy * scale), dim=1).contiguous()

    def _detect_and_branch(self, img, branch):
        """One image of ``predict`` / ``predict_keypoints`` (inference mode set by the caller): the detections and, with ``branch`` and
        D > 0, the mask / keypoint branch on the kept boxes.  Returns (size, bbox (D,4) contiguous, label, score, m, mirrors): without
        test-time augmentation m = the branch output (D,S,S,C) and mirrors = None; with it m = one such output per view and mirrors =
        the views' mirror flags; m = None where the branch did not run."""
        if self.tta is not None:
            size, bbox, label, score, level, view, views = self._detect_tta(img)
            bbox = bbox.contiguous()
            m = self._branch_per_view(bbox, level, view, views, size[1]) if branch and bbox.shape[0] > 0 else None
            return size, bbox, label, score, m, [v[2] for v in views]
        size, scale, bbox, label, score, level = self._detect(img)
        bbox = bbox.contiguous()
        m = None
        if branch and bbox.shape[0] > 0:        # not through _branch_per_view: the one view's levels are the proposals' own
            m = self.head.mask_branch(self.head.x, self._xy5(bbox, scale), level.to(torch.int32).contiguous(),
                                      self.extractor.spatial_scales)
        self._box_score = score
        self.last_maskiou = None
        self.last_point_grid = self.last_point_coarse = None
        if m is not None and self.point_head is not None and self.predict_mask:
            self.last_point_coarse = m
            if self.point_rend_refine:
                self.last_point_grid = self._point_refine(m, self._xy5(bbox, scale), label.to(torch.int32).contiguous())
        if m is not None and self.maskiou_head is not None and self.predict_mask:
            # Mask Scoring R-CNN: the MaskIoU head on the kept detections, behind the mask branch and behind _suppress -
            # the order, the count, the boxes and the masks of the detections are those of the box scores (use_max_detections included)
            mh = self.maskiou_head
            lab = label.to(torch.int32).contiguous()
            x_in = mh.assemble(self.head.last_mask_pool, m, lab, label_base=0)
            pred = mh.forward(x_in)
            self.last_maskiou = (x_in, pred)        # parity tests read these
            if self.mask_iou_rescore:
                score = ops.maskiou_rescore(score.to(torch.float32).contiguous(), pred, lab, mh.out_channels)
        return size, bbox, label, score, m, None

    def _point_refine(self, m, rois_xy5, label):
        """PointRend inference on the coarse logits m (D,S0,S0,Cp) of the detections with boxes ``rois_xy5`` (the forward's
        frame) and 0-based labels: per subdivision step a 2x upsample of the class's grid, the most uncertain cells, the point head on their
        centres - fine features from the pyramid kept in ``head.x``, coarse features from the ORIGINAL logits - and their predictions written
        over those cells.  Returns the (D,G,G) logit grid, G = S0 * 2^steps."""
        ph, st = self.point_head, self.point_rend
        grid, lab = m, label
        scale0 = self.extractor.spatial_scales[0]
        for _ in range(st['subdivision_steps']):
            up, index, coords = ops.point_subdivide(grid, lab, ph.out_channels if lab is not None else 1, st['subdivision_points'])
            x_in = ph.assemble(coords, rois_xy5, self.head.x[0], scale0, m)
            pred = ph.forward(x_in)
            ops.point_scatter(pred, label, index, ph.out_channels, up)
            grid, lab = up.view(up.shape[0], up.shape[1], up.shape[2], 1), None
        return grid.view(grid.shape[0], grid.shape[1], grid.shape[2])

    def predict(self, imgs):
        """maskrcnn.py:157-259: imgs = list of (3,H,W) float32 tensors (0..255).  Returns (masks, labels, scores) -
        lists with one entry per image: masks (D,H,W) bool, labels (D,) int32 in [0, n_fg_class-1], scores (D,) float32 -
        and keeps the boxes in ``self.last_bboxes``.  One device->host copy per image (the per-class keep counts).  On a ``mask_iou`` model
        the scores are box score x predicted mask IoU (unless ``mask_iou_rescore`` is False); ``self.last_box_scores`` keeps the box scores."""
        masks, labels, scores, bboxes, box_scores = [], [], [], [], []
        with self._inference_mode():
            for img in imgs:
                size, bbox, label, score, m, mirrors = self._detect_and_branch(img, self.predict_mask)
                box_scores.append(score if mirrors is not None else self._box_score)
                if m is None:
                    mask = torch.zeros((bbox.shape[0],) + size, dtype=torch.bool, device=self.device)
                elif mirrors is None and self.last_point_grid is not None:
                    # the refined grid through the unchanged paste rule: one channel, so every detection's label is 0
                    g = self.last_point_grid
                    mask = ops.mask_paste(g.view(g.shape[0], g.shape[1], g.shape[2], 1), torch.zeros_like(label, dtype=torch.int32), bbox,
                                          size).bool()
                elif mirrors is None:
                    mask = ops.mask_paste(m, label.contiguous(), bbox, size).bool()
                else:
                    mask = ops.mask_paste_prob(ops.tta_mask_merge(m, mirrors, label.contiguous()), bbox, size).bool()
                masks.append(mask)
                labels.append(label)
                scores.append(score)
                bboxes.append(bbox)
        self.last_bboxes = bboxes
        self.last_box_scores = box_scores       # the scores before the MaskIoU rescoring (the same tensors without a MaskIoU head)
        return masks, labels, scores

    def _detect(self, img):
        """The detection part of ``predict`` for one image (inference mode set by the caller): prepare, forward, box decode and
        per-class NMS.  Returns (size, scale, bbox (D,4) in image coordinates, label, score, level)."""
        size = tuple(img.shape[1:])
        x = self.prepare(img.to(self.device))
        scale = x.shape[2] / size[1]
        roi_cls_locs, roi_scores, rois, roi_indices, levels = self.__call__(x[None].contiguous(), scale=scale)
        box_out = self.head.last_box_out
        rois = rois.contiguous()
        self.last_stages = [(rois, box_out)]        # parity tests read these: every box stage's (input boxes, box_out)
        std = self.loc_normalize_std
        if self.cascade is not None:
            # stage k's input = stage k-1's decoded boxes, clipped to the prepared image (the forward's frame), on the pyramid kept in head.x
            frame = (float(x.shape[1]), float(x.shape[2]))
            stds = self.cascade_stds
            for k, stage in enumerate(self.cascade_heads, 1):
                ref = ops.cascade_refine(rois, box_out, self.head.LOC0, 1, self.loc_normalize_mean, stds[k - 1], frame)
                rois, levels = ref['roi'], ref['levels']
                box_out = stage.box_branch(self.head.x, ref['rois_xy5'], levels, self.extractor.spatial_scales)
                self.last_stages.append((rois, box_out))
            std = stds[-1]
        cls_bbox, prob = ops.detect_decode(rois, box_out, self.n_class, self.head.LOC0, scale, self.loc_normalize_mean, std, size)
        if self.cascade is not None:
            prob = ops.cascade_prob([b for _, b in self.last_stages], self.n_class)
        self.last_rois, self.last_decoded = rois, (cls_bbox, prob)      # parity tests read these
        bbox, label, score, level = self._suppress(cls_bbox, prob, levels)
        return size, scale, bbox, label, score, level

    def _detect_tta(self, img):
        """``_detect`` over the test-time views: per view the mirrored / resized image and its own N = 1 forward (features kept), then ONE
        decode of all views' candidates (mirrored boxes mapped back) and the class NMS over their union.  Returns (size, bbox, label, score,
        level, view, views): level / view = the proposal level and the view of each kept detection; views = [(features, scale, mirror)]."""
        size = tuple(img.shape[1:])
        H, W = size
        src = img.to(self.device, torch.float32).contiguous()
        views, rois_v, box_v, level_v = [], [], [], []
        for oh, ow, mirror in self.test_views(H, W):
            x = ops.image_resize_mirror_f32(src, oh, ow, int(mirror), 255.0)
            scale = x.shape[2] / W
            _, _, rois, _, levels = self.__call__(x[None].contiguous(), scale=scale)
            views.append((self.head.x, scale, mirror))
            rois_v.append(rois.contiguous())
            box_v.append(self.head.last_box_out)
            level_v.append(levels)
        cls_bbox, prob = ops.tta_detect_decode(rois_v, box_v, [v[2] for v in views], [v[1] for v in views], self.n_class, self.head.LOC0,
                                               self.loc_normalize_mean, self.loc_normalize_std, size)
        self.last_rois, self.last_decoded = rois_v, (cls_bbox, prob)
        view = torch.cat([torch.full((r.shape[0],), v, dtype=torch.int32, device=self.device) for v, r in enumerate(rois_v)])
        bbox, label, score, level, view = self._suppress(cls_bbox, prob, torch.cat(level_v), view=view)
        return size, bbox, label, score, level, view, views

    def _branch_per_view(self, bbox, level, view, views, W):
        """The mask / keypoint branch of every view on the final boxes bbox (D,4) (original image): mirrored into a mirrored view, scaled
        by the view's scale; a detection keeps its proposal's level in its own view and takes map_rois_to_fpn_levels of the box in every
        other view.  Returns the per-view branch outputs (D,S,S,C)."""
        out = []
        for u, (feats, scale, mirror) in enumerate(views):
            b = torch.stack((bbox[:, 0], W - bbox[:, 3], bbox[:, 2], W - bbox[:, 1]), dim=1) if mirror else bbox
            b = b * scale
            lv = torch.where(view == u, level, ops.map_rois_to_fpn_levels(b.contiguous()).clamp(0, len(feats) - 1))
            out.append(self.head.mask_branch(feats, self._xy5(b), lv.to(torch.int32).contiguous(), self.extractor.spatial_scales))
        return out

    def predict_keypoints(self, imgs, return_heatmaps=False):
        """Keypoint R-CNN inference (head_arch 'fpn_keypoint'): the detections of ``predict`` (same prepare / forward / decode /
        NMS, boxes kept in ``self.last_bboxes``), then the keypoint branch on the kept boxes and ``mrcnn_keypoint_decode_f32``.
        Returns (keypoints, labels, scores), one entry per image: keypoints (D,K,4) float32 (y, x, logit, prob) on the device, y / x
        in the image coordinates of the boxes (the top-left corner of the argmax cell of the 56 x 56 map, the reference viewer's
        rule, viewer.py:86-107), prob = the softmax over the cells at the argmax.  return_heatmaps=True appends the heat maps in the
        reference's format (maskrcnn.py:249: (D, K, 56*56), there with a fixed 20 for K).  Like ``predict``, one device->host copy
        per image (the per-class keep counts)."""
        if self.head_arch != 'fpn_keypoint':
            raise ValueError('predict_keypoints needs a keypoint model (head_arch \'fpn_keypoint\'), this one has %r' % self.head_arch)
        K, S = self.head.n_keypoints, self.head.mask_size
        keypoints, labels, scores, bboxes, heatmaps = [], [], [], [], []
        with self._inference_mode():
            for img in imgs:
                size, bbox, label, score, m, mirrors = self._detect_and_branch(img, True)
                D = bbox.shape[0]
                if m is None:                   # D = 0
                    m = torch.zeros((0, S, S, K), dtype=torch.float32, device=self.device)
                    kp = torch.zeros((0, K, 4), dtype=torch.float32, device=self.device)
                else:
                    if mirrors is not None:
                        m = ops.tta_keypoint_merge(m, mirrors, K, self.tta['keypoint_flip_perm'])
                    kp = ops.keypoint_decode(m, bbox, K)
                keypoints.append(kp)
                labels.append(label)
                scores.append(score)
                bboxes.append(bbox)
                if return_heatmaps:
                    heatmaps.append(m[..., :K].permute(0, 3, 1, 2).reshape(D, K, S * S))
        self.last_bboxes = bboxes
        if return_heatmaps:
            return keypoints, labels, scores, heatmaps
        return keypoints, labels, scores

    def _suppress(self, cls_bbox, prob, levels, view=None):
        """maskrcnn.py:278-312 on the device: for every foreground class l (skipping the LAST class when masks are
        predicted - the reference's off-by-one guard, :288-291): prob[:, l] > score_thresh, NMS(nms_thresh) in
        descending score order; results concatenated over classes, labels l-1.  Returns (bbox, label, score, level) of the kept
        rows, and with ``view`` (the test-time views' union, up to 4096 candidates) the kept rows of ``view`` last.

        Optional stages, none of which launches anything when off: with ``soft_nms`` the selection runs through
        class_soft_nms and its decayed scores are the returned ones; with ``vote_thresh`` the kept boxes go through box_vote; with
        ``max_detections`` the cap highest scores (ties to the earlier row) stay, in their order.  level / view are always those of
        the kept proposal.  One host sync: the keep counts."""
        dev = prob.device
        l_end = self.n_class - 1 if self.predict_mask else self.n_class
        soft, vote, cap = self.soft_nms, self.vote_thresh, self.max_detections
        keep_score = keep_box = None
        if soft is not None:
            keep_idx, keep_score, keep_cnt = ops.class_soft_nms(cls_bbox, prob, 1, l_end, self.score_thresh, soft[0], self.nms_thresh, soft[1])
        else:                                           # (up to 512 rows class_nms_ws runs class_nms's kernel and takes no workspace)
            keep_idx, keep_cnt = ops.class_nms_ws(cls_bbox, prob, 1, l_end, self.score_thresh, self.nms_thresh)
        if vote is not None:
            keep_box = ops.box_vote(cls_bbox, prob, 1, l_end, self.score_thresh, vote, keep_idx, keep_cnt)
        cnt = keep_cnt.cpu().tolist()                   # the one host sync of predict()
        kept = [l for l in range(1, l_end) if cnt[l]]
        if not kept:
            sel = torch.zeros((0,), dtype=torch.long, device=dev)
            out = (cls_bbox[sel], sel.to(torch.int32), prob[sel, 0])
        else:
            rows = lambda t: torch.cat([t[l, :cnt[l]] for l in kept])       # the kept entries of a per-class (n_class, R, ...) output
            lab = [torch.full((cnt[l],), l - 1, dtype=torch.int32, device=dev) for l in kept]
            sel = rows(keep_idx).long()
            lab = torch.cat(lab)
            bbox = cls_bbox[sel] if keep_box is None else rows(keep_box)
            score = prob[sel, (lab + 1).long()] if keep_score is None else rows(keep_score)
            if cap is not None and sel.shape[0] > cap:
                top = torch.sort(score, descending=True, stable=True)[1][:cap]
                top = torch.sort(top)[0]
                sel, lab, score, bbox = sel[top], lab[top], score[top], bbox[top]
            out = (bbox, lab, score)
        out += (levels[sel],)
        return out if view is None else out + (view[sel],)

    def prepare_size(self, H, W):
        """Scaled size of maskrcnn.py:261-271 (min side -> min_size unless the max side would exceed max_size)."""
        return scaled_size(H, W, self.min_size, self.max_size)


def scaled_size(H, W, min_size, max_size):
    """maskrcnn.py:261-271: the size of an H x W image whose short side goes to min_size unless the long side would exceed max_size."""
    scale = min_size / min(H, W)
    if scale * max(H, W) > max_size:
        scale = max_size / max(H, W)
    return int(H * scale), int(W * scale)
