"""The inference options of the entry scripts, stated once: the test-time augmentation and box post-processing flags of evaluate.py and
demo.py (train.py declares them with the prefix '--eval-' for its periodic evaluator), what they turn into on a model, the table of the
optional model extensions that all four scripts walk (EXTENSIONS), the deformable-convolution flags beside it, the label file and the
model a checkpoint is scored or drawn with.
Importing this module needs neither a device nor the training script."""
import collections
import os

DEFAULT_SOFT_NMS_SIGMA = 0.5        # --soft-nms-sigma when not given (Detectron's TEST.SOFT_NMS.SIGMA)


# ---- test-time augmentation (MaskRCNN.use_test_augmentation) ------------------------------------------------------------
def add_tta_flags(parser, prefix='--'):
    """--tta-sizes / --tta-hflip / --tta-max-size of evaluate.py and demo.py; with the prefix '--eval-' the flags of train.py's periodic
    evaluator."""
    parser.add_argument(prefix + 'tta-sizes', type=int, nargs='+', default=None, metavar='N',
                        help='test-time augmentation (MaskRCNN.use_test_augmentation): run every image at these short sides and merge '
                             'the views; off by default')
    parser.add_argument(prefix + 'tta-hflip', type=int, default=0, choices=[0, 1],
                        help='1: test-time augmentation adds the mirrored view of every size (the model\'s min_size when no %stta-sizes); '
                             'keypoint heads swap their left / right channels' % prefix)
    parser.add_argument(prefix + 'tta-max-size', type=int, default=None,
                        help='long-side cap of the test-time views (default: the model\'s max_size)')


def tta_settings(sizes, hflip, max_size, min_size):
    """use_test_augmentation's arguments from the TTA flags (--tta-* of evaluate.py, --eval-tta-* of train.py): None = off.  hflip without
    sizes mirrors the model's own min_size."""
    if not sizes and not hflip:
        if max_size is not None:
            raise ValueError('a test-time max size needs test-time sizes or the test-time flip')
        return None
    return {'sizes': [int(s) for s in sizes] if sizes else [int(min_size)], 'hflip': bool(hflip),
            'max_size': None if max_size is None else int(max_size)}


def use_tta(model, settings, keypoint_names=None, prefix='--'):
    """Applies tta_settings' result (None: nothing) to the model.  A keypoint head with hflip swaps its left / right channels by the flip
    permutation of ``keypoint_names`` (default: COCO's 17 names); ValueError, naming the flag ``prefix``tta-hflip, when they are not the
    head's keypoints or do not pair."""
    if settings is None:
        return
    perm = None
    if model.head_arch == 'fpn_keypoint' and settings['hflip']:
        from chainer_maskrcnn.dataset import augment
        names = augment.COCO_KEYPOINT_NAMES if keypoint_names is None else keypoint_names
        if len(names) != model.head.n_keypoints:
            raise ValueError('%stta-hflip 1: %d keypoint names for %d keypoints' % (prefix, len(names), model.head.n_keypoints))
        try:
            perm = augment.flip_permutation(names)
        except ValueError as e:
            raise ValueError('%stta-hflip 1: this keypoint dataset has no complete left / right flip map (%s)' % (prefix, e))
    model.use_test_augmentation(settings['sizes'], hflip=settings['hflip'], max_size=settings['max_size'], keypoint_flip_perm=perm)


# ---- box post-processing (MaskRCNN.use_soft_nms / use_box_voting / use_max_detections) ----------------------------------
def add_boxpost_flags(parser, prefix='--'):
    """--soft-nms / --soft-nms-sigma / --box-vote-thresh / --max-detections of evaluate.py and demo.py; with the prefix '--eval-' the
    flags of train.py's periodic evaluator."""
    parser.add_argument(prefix + 'soft-nms', default='off', choices=['off', 'linear', 'gaussian'],
                        help='Soft-NMS in place of the hard per-class NMS (MaskRCNN.use_soft_nms): a kept box lowers the scores of the '
                             'boxes it overlaps instead of deleting them; off by default')
    parser.add_argument(prefix + 'soft-nms-sigma', type=float, default=None, metavar='S',
                        help='sigma of %ssoft-nms gaussian (default %s)' % (prefix, DEFAULT_SOFT_NMS_SIGMA))
    parser.add_argument(prefix + 'box-vote-thresh', type=float, default=0.0, metavar='T',
                        help='box voting (MaskRCNN.use_box_voting): every kept box becomes the score-weighted mean of the candidates of '
                             'its class with IoU >= T (Detectron: 0.8); 0 = off')
    parser.add_argument(prefix + 'max-detections', type=int, default=0, metavar='N',
                        help='keep the N highest-scoring detections of an image (MaskRCNN.use_max_detections; Detectron: 100); 0 = off')


def boxpost_settings(soft_nms, sigma, vote_thresh, max_detections, prefix='--'):
    """The arguments of use_soft_nms / use_box_voting / use_max_detections from the flags (evaluate.py, demo.py; --eval-* of train.py):
    None = all off, else {'soft_nms': None | 'linear' | 'gaussian', 'sigma', 'vote_thresh': None | T, 'max_detections': None | N}.
    ValueError for a value the model would refuse."""
    if soft_nms not in ('off', 'linear', 'gaussian'):
        raise ValueError('%ssoft-nms must be off, linear or gaussian, got %r' % (prefix, soft_nms))
    if sigma is not None and soft_nms != 'gaussian':
        raise ValueError('%ssoft-nms-sigma belongs to %ssoft-nms gaussian' % (prefix, prefix))
    if sigma is not None and not sigma > 0:
        raise ValueError('%ssoft-nms-sigma must be positive, got %r' % (prefix, sigma))
    if not 0 <= vote_thresh <= 1:
        raise ValueError('%sbox-vote-thresh must lie in (0, 1] (0 = off), got %r' % (prefix, vote_thresh))
    if max_detections < 0:
        raise ValueError('%smax-detections must not be negative (0 = off), got %r' % (prefix, max_detections))
    if soft_nms == 'off' and not vote_thresh and not max_detections:
        return None
    return {'soft_nms': None if soft_nms == 'off' else soft_nms, 'sigma': float(sigma) if sigma is not None else DEFAULT_SOFT_NMS_SIGMA,
            'vote_thresh': float(vote_thresh) if vote_thresh else None, 'max_detections': int(max_detections) if max_detections else None}


def add_boundary_flag(parser, prefix='--'):
    """--boundary of evaluate.py; with the prefix '--eval-' the flag of train.py's periodic evaluator (--eval-boundary)."""
    parser.add_argument(prefix + 'boundary', type=int, default=0, choices=[0, 1],
                        help='1: also report Boundary AP (Cheng et al., CVPR 2021): COCO mask AP with min(mask IoU, IoU of the masks\' '
                             'boundary bands) as the IoU (InstanceSegmentationCOCOEvaluator iou_types); off by default')


def boundary_iou_types(boundary, eval_metric='mask_coco', keypoints=False, prefix='--'):
    """The COCO evaluator's iou_types from the flag (--boundary of evaluate.py; --eval-boundary of train.py, which needs --eval-metric
    mask_coco and a mask head).  ValueError for a combination that has no Boundary AP."""
    flag = prefix + 'boundary'
    if boundary not in (0, 1):
        raise ValueError('%s must be 0 or 1, got %r' % (flag, boundary))
    if not boundary:
        return ('segm', 'bbox')
    if keypoints:
        raise ValueError('%s 1: Boundary AP is a mask metric; keypoint heads (train_keypoints.py) have none' % flag)
    if eval_metric != 'mask_coco':
        raise ValueError('%s 1: Boundary AP is computed by the COCO evaluator; it needs --eval-metric mask_coco, not %s' % (flag, eval_metric))
    return ('segm', 'bbox', 'boundary')


def use_boxpost(model, settings):
    """Applies boxpost_settings' result (None: nothing) to the model."""
    if settings is None:
        return
    model.use_soft_nms(settings['soft_nms'], settings['sigma'])
    model.use_box_voting(settings['vote_thresh'])
    model.use_max_detections(settings['max_detections'])


# ---- head normalisation -------------------------------------------------------------------------------------------------------------------
def add_head_norm_flags(parser, both=lambda name: (name,)):
    """--head-norm / --gn-groups (train.py, train_keypoints.py - which takes both spellings through ``both`` -, evaluate.py, demo.py)."""
    parser.add_argument(*both('--head-norm'), default='none', choices=['none', 'gn'],
                        help='gn: GroupNorm behind conv1 and every mask / keypoint convolution of the FPN heads (MaskRCNN head_norm; '
                             'Detectron\'s *_gn heads), for long schedules from scratch; a checkpoint is evaluated with the value it was '
                             'trained with')
    parser.add_argument(*both('--gn-groups'), type=int, default=32, metavar='G', help='groups of --head-norm gn; must divide the head\'s 256 channels')


def head_norm_settings(head_norm, gn_groups, head_arch):
    """The MaskRCNN arguments {'head_norm': None | 'gn', 'gn_groups': G} of the flags; ValueError for a combination the model refuses."""
    if head_norm not in ('none', 'gn'):
        raise ValueError('--head-norm must be none or gn, got %r' % (head_norm,))
    if head_norm == 'gn' and head_arch in ('res5', 'light'):
        raise ValueError('--head-norm gn exists for --head-arch fpn and fpn_keypoint, not %s' % head_arch)
    if gn_groups < 1 or (head_norm == 'gn' and 256 % gn_groups != 0):
        raise ValueError('--gn-groups must be a positive divisor of the head\'s 256 channels, got %r' % (gn_groups,))
    return {'head_norm': None if head_norm == 'none' else head_norm, 'gn_groups': int(gn_groups)}


# ---- FPN normalisation (MaskRCNN fpn_norm) --------------------------------------------------------------------------------
def add_fpn_norm_flags(parser, both=lambda name: (name,)):
    """--fpn-norm (train.py, train_keypoints.py - which takes both spellings through ``both`` -, evaluate.py, demo.py); its groups are
    --gn-groups, shared with --head-norm."""
    parser.add_argument(*both('--fpn-norm'), default='none', choices=['none', 'gn'],
                        help='gn: GroupNorm of --gn-groups groups behind each of the eight FPN convolutions (MaskRCNN fpn_norm; Detectron\'s '
                             '*_gn configurations normalise the FPN and the heads together), for long schedules from scratch; --backbone fpn '
                             'only; a checkpoint is evaluated with the value it was trained with')


def fpn_norm_settings(fpn_norm, gn_groups, backbone):
    """The MaskRCNN argument {'fpn_norm': None | 'gn'} of the flags; ValueError for a combination the model refuses."""
    if fpn_norm not in ('none', 'gn'):
        raise ValueError('--fpn-norm must be none or gn, got %r' % (fpn_norm,))
    if fpn_norm == 'gn' and backbone != 'fpn':
        raise ValueError('--fpn-norm gn exists for --backbone fpn, not %s' % backbone)
    if fpn_norm == 'gn' and (gn_groups < 1 or 256 % gn_groups != 0):
        raise ValueError('--gn-groups must be a positive divisor of the FPN\'s 256 channels, got %r' % (gn_groups,))
    return {'fpn_norm': None if fpn_norm == 'none' else fpn_norm}


# ---- Cascade R-CNN box stages (MaskRCNN cascade_ious / cascade_stds) -------------------------------------------------------
DEFAULT_CASCADE_IOUS = (0.5, 0.6, 0.7)
NO_CASCADE = {'cascade_ious': None, 'cascade_stds': None}       # what a trainer state without the 'cascade' key was trained with


def add_cascade_flags(parser, both=lambda name: (name,)):
    """--cascade / --cascade-ious / --cascade-stds (train.py, train_keypoints.py - which takes both spellings through ``both`` -, evaluate.py,
    demo.py)."""
    parser.add_argument(*both('--cascade'), type=int, default=0, choices=[0, 1],
                        help='1: Cascade R-CNN - the box head becomes K stages trained at rising IoU thresholds, each fed the boxes the stage '
                             'before refined, their scores averaged at inference (MaskRCNN cascade_ious); a checkpoint is evaluated with the '
                             'value it was trained with')
    parser.add_argument(*both('--cascade-ious'), type=float, nargs='+', default=None, metavar='T',
                        help='the IoU thresholds of --cascade 1, one per stage (2 to 4, not decreasing, the first 0.5); default %s'
                             % ' '.join(str(v) for v in DEFAULT_CASCADE_IOUS))
    parser.add_argument(*both('--cascade-stds'), type=float, nargs='+', default=None, metavar='S',
                        help='the delta normalisation of the stages behind the first, 4 numbers each (default: 0.05 0.05 0.1 0.1  0.033 0.033 '
                             '0.067 0.067; other stage counts: the first stage\'s divided by the stage number)')


def cascade_flag_settings(cascade, ious, stds, head_arch, backbone='fpn'):
    """The MaskRCNN arguments {'cascade_ious': None | tuple, 'cascade_stds': None | tuple of 4-tuples} of the flags; ValueError for a
    combination the model refuses."""
    if cascade not in (0, 1):
        raise ValueError('--cascade must be 0 or 1, got %r' % (cascade,))
    if not cascade:
        if ious is not None or stds is not None:
            raise ValueError('--cascade-ious / --cascade-stds belong to --cascade 1')
        return dict(NO_CASCADE)
    from chainer_maskrcnn.model.maskrcnn import cascade_settings
    ious = tuple(float(v) for v in ious) if ious else DEFAULT_CASCADE_IOUS
    if stds is not None:
        if len(stds) % 4 or len(stds) // 4 not in (len(ious) - 1, len(ious)):
            raise ValueError('--cascade-stds takes 4 numbers for each of the %d stages behind the first, got %d numbers' % (len(ious) - 1, len(stds)))
        stds = tuple(tuple(float(v) for v in stds[i:i + 4]) for i in range(0, len(stds), 4))
    try:
        got = cascade_settings(ious, stds, head_arch, backbone)
    except ValueError as e:
        raise ValueError('--cascade 1: %s' % e)
    return {'cascade_ious': got[0], 'cascade_stds': got[1]}


# ---- Mask Scoring R-CNN (MaskRCNN mask_iou, FPNMaskRCNNTrainChain mask_iou_weight) ----------------------------------------
NO_MASK_IOU = {'mask_iou': False, 'mask_iou_weight': 1.0}       # what a trainer state without the 'mask_iou' key was trained with


def add_mask_iou_flags(parser, both=lambda name: (name,), weight=False):
    """--mask-iou (train.py, evaluate.py, demo.py; train_keypoints.py takes it to refuse it) and, with ``weight``, --mask-iou-weight
    (the training scripts)."""
    parser.add_argument(*both('--mask-iou'), type=int, default=0, choices=[0, 1],
                        help='1: Mask Scoring R-CNN - a MaskIoU head regresses the IoU of every predicted mask with its ground truth and '
                             'inference ranks a detection by box score x predicted mask IoU (MaskRCNN mask_iou; --head-arch fpn only); a '
                             'checkpoint is evaluated with the value it was trained with')
    if weight:
        parser.add_argument(*both('--mask-iou-weight'), type=float, default=None, metavar='W',
                            help='the weight of the MaskIoU head\'s L2 loss under --mask-iou 1 (default 1.0)')


def mask_iou_settings(mask_iou, weight=None, head_arch='fpn'):
    """{'mask_iou': bool, 'mask_iou_weight': float} of the flags; ValueError for a combination the model or the training chain refuses."""
    from chainer_maskrcnn.model.maskrcnn import mask_iou_setting
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import mask_iou_weight_setting
    if mask_iou not in (0, 1):
        raise ValueError('--mask-iou must be 0 or 1, got %r' % (mask_iou,))
    if not mask_iou:
        if weight is not None:
            raise ValueError('--mask-iou-weight belongs to --mask-iou 1')
        return dict(NO_MASK_IOU)
    try:
        on = mask_iou_setting(bool(mask_iou), head_arch)
        w = mask_iou_weight_setting(1.0 if weight is None else weight)
    except ValueError as e:
        raise ValueError('--mask-iou 1: %s' % e)
    return {'mask_iou': on, 'mask_iou_weight': w}


# ---- PointRend (MaskRCNN point_rend ..., FPNMaskRCNNTrainChain point_loss_weight) ------------------------------------------
POINT_SHAPE_DEFAULTS = {'point_train_points': 196, 'point_oversample': 3, 'point_importance': 0.75, 'subdivision_steps': 2,
                        'subdivision_points': 784}
# what a trainer state without the 'point_rend' key was trained with
NO_POINT_REND = dict({'point_rend': False, 'point_loss_weight': 1.0}, **POINT_SHAPE_DEFAULTS)


def add_point_rend_flags(parser, both=lambda name: (name,), weight=False):
    """--point-rend and its five shape flags (train.py, evaluate.py, demo.py; train_keypoints.py takes them to refuse them) and, with
    ``weight``, --point-loss-weight (the training scripts)."""
    parser.add_argument(*both('--point-rend'), type=int, default=0, choices=[0, 1],
                        help='1: PointRend - a point head predicts the mask at single points from the stride-4 level and the coarse logits; '
                             'inference refines the 28 x 28 mask by subdivision (MaskRCNN point_rend; --head-arch fpn only, not with '
                             '--mask-iou); a checkpoint is evaluated with the values it was trained with')
    parser.add_argument(*both('--point-train-points'), type=int, default=None, metavar='P',
                        help='--point-rend 1: training points per mask row (default %d)' % POINT_SHAPE_DEFAULTS['point_train_points'])
    parser.add_argument(*both('--point-oversample'), type=int, default=None, metavar='K',
                        help='--point-rend 1: candidates per training point (default %d)' % POINT_SHAPE_DEFAULTS['point_oversample'])
    parser.add_argument(*both('--point-importance'), type=float, default=None, metavar='BETA',
                        help='--point-rend 1: the share of the training points taken from the most uncertain candidates (default %s)'
                             % POINT_SHAPE_DEFAULTS['point_importance'])
    parser.add_argument(*both('--subdivision-steps'), type=int, default=None, metavar='N',
                        help='--point-rend 1: 2x subdivision steps at inference, 1 or 2 (default %d)' % POINT_SHAPE_DEFAULTS['subdivision_steps'])
    parser.add_argument(*both('--subdivision-points'), type=int, default=None, metavar='N',
                        help='--point-rend 1: cells re-predicted per detection and step (default %d)' % POINT_SHAPE_DEFAULTS['subdivision_points'])
    if weight:
        parser.add_argument(*both('--point-loss-weight'), type=float, default=None, metavar='W',
                            help='the weight of the point loss under --point-rend 1 (default 1.0)')


def point_rend_flag_settings(args, head_arch='fpn', mask_iou=0, weight=False):
    """The PointRend settings of the flags as a dict with NO_POINT_REND's keys; ValueError for a shape flag or a weight without
    --point-rend 1 and for a combination the model or the training chain refuses."""
    from chainer_maskrcnn.model.maskrcnn import point_rend_settings
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import point_loss_weight_setting
    on = getattr(args, 'point_rend', 0)
    if on not in (0, 1):
        raise ValueError('--point-rend must be 0 or 1, got %r' % (on,))
    given = {k: getattr(args, k, None) for k in POINT_SHAPE_DEFAULTS}
    w = getattr(args, 'point_loss_weight', None) if weight else None
    if not on:
        extra = [k for k, v in given.items() if v is not None] + (['point_loss_weight'] if w is not None else [])
        if extra:
            raise ValueError('--%s belongs to --point-rend 1' % extra[0].replace('_', '-'))
        return dict(NO_POINT_REND)
    shape = {k: (POINT_SHAPE_DEFAULTS[k] if v is None else v) for k, v in given.items()}
    try:
        point_rend_settings(True, head_arch=head_arch, mask_iou=bool(mask_iou), **shape)
        w = point_loss_weight_setting(1.0 if w is None else w)
    except ValueError as e:
        raise ValueError('--point-rend 1: %s' % e)
    return dict({'point_rend': True, 'point_loss_weight': w}, **shape)


def point_rend_model_kwargs(settings):
    """The MaskRCNN keyword arguments of point_rend_flag_settings' dict (nothing when it is off: a default model)."""
    if not settings['point_rend']:
        return {}
    return dict({'point_rend': True}, **{k: settings[k] for k in POINT_SHAPE_DEFAULTS})


# ---- deformable convolution in res3-res5 (MaskRCNN dcn_stages / dcn_modulated) ------------------------------------------------
# Beside the table below, like train.py's freeze and box-loss flags: the two MaskRCNN arguments are passed only when --dcn-stages is given.
NO_DCN = {'stages': [], 'modulated': False}        # what a trainer state without the 'dcn' key was trained with
DCN_NOUN = 'the deformable convolution settings'    # the noun of the --resume refusal


def add_dcn_flags(parser, both=lambda name: (name,)):
    """--dcn-stages / --dcn-modulated (train.py, train_keypoints.py - which takes both spellings through ``both`` -, evaluate.py, demo.py)."""
    parser.add_argument(*both('--dcn-stages'), nargs='+', default=None, metavar='STAGE',
                        help='deformable convolution (MaskRCNN dcn_stages): every bottleneck of these stages among res3 res4 res5 runs its 3x3 '
                             'layer as a deformable convolution (the dconv_c3-c5 configurations name all three); --backbone fpn only; a '
                             'checkpoint is evaluated with the value it was trained with; no accuracy effect has been measured; off by default')
    parser.add_argument(*both('--dcn-modulated'), type=int, default=0, choices=[0, 1],
                        help='1: the modulated form (v2, the mdconv_c3-c5 configurations): every sample is scaled by a learned mask; needs '
                             '--dcn-stages')


def dcn_settings(stages, modulated, backbone='fpn'):
    """{'stages': the stages in network order ([] = off), 'modulated': bool} of the flags, as trainer_<it>.pt records it; ValueError, before
    any device work, for what MaskRCNN refuses (maskrcnn.dcn_settings states it): an unknown stage name, --dcn-modulated 1 without
    --dcn-stages, another --backbone."""
    from chainer_maskrcnn.model.maskrcnn import dcn_settings as model_rule
    try:
        got = model_rule(tuple(stages) if stages else None, modulated, backbone)
    except ValueError as e:
        raise ValueError('--dcn-stages / --dcn-modulated: %s' % e)
    return {'stages': list(got[0]), 'modulated': got[1]}


def dcn_model_kwargs(settings):
    """The MaskRCNN keyword arguments of dcn_settings' dict (nothing when it is off: a default model)."""
    if not settings['stages']:
        return {}
    return {'dcn_stages': tuple(settings['stages']), 'dcn_modulated': bool(settings['modulated'])}


def dcn_settings_of(args):
    """dcn_settings of a script's parsed flags."""
    return dcn_settings(getattr(args, 'dcn_stages', None), getattr(args, 'dcn_modulated', 0), args.backbone)


# ---- the optional model extensions, declared once for train.py, train_keypoints.py, evaluate.py and demo.py --------------------------------
# One record per extension, holding what the scripts' glue differs in:
#   add_flags(parser, both[, weight]) declares its flags; weight_flag names the one that only the training scripts take
#   settings(args, training) is its settings dict from parsed flags (ValueError for what the model refuses), is_on(settings) tells whether it is on
#   off is that dict with the flags off, state_key its key in trainer_<it>.pt (a state without the key was trained with ``off``)
#   the two norms have neither: trainer_<it>.pt has never recorded them, and that is kept
#   switch turns it on; with model_noun and settings_noun it words the refusals; refuses_tta: MaskRCNN.use_test_augmentation refuses it
#   mask_heads_only: (asked(args), the sentence keypoint training refuses it with)
#   model_kwargs(settings) are the MaskRCNN arguments it contributes, chain_keys the settings FPNMaskRCNNTrainChain takes, loss_key what it logs
Extension = collections.namedtuple('Extension', 'name add_flags settings is_on weight_flag off state_key switch model_noun settings_noun refuses_tta '
                                                'mask_heads_only model_kwargs chain_keys loss_key',
                                   defaults=(None, None, None, None, None, None, False, None, dict, (), None))


def _cascade_settings_of(args, training):
    s = cascade_flag_settings(args.cascade, args.cascade_ious, args.cascade_stds, args.head_arch, args.backbone)
    if training:        # trainer_<it>.pt records lists
        s = {k: None if v is None else [list(x) if isinstance(x, tuple) else x for x in v] for k, v in s.items()}
    return s


EXTENSIONS = (
    Extension('head_norm', add_head_norm_flags, lambda a, training: head_norm_settings(a.head_norm, a.gn_groups, a.head_arch),
              is_on=lambda s: s['head_norm'] is not None, switch='--head-norm gn'),
    Extension('fpn_norm', add_fpn_norm_flags, lambda a, training: fpn_norm_settings(a.fpn_norm, a.gn_groups, a.backbone),
              is_on=lambda s: s['fpn_norm'] is not None, switch='--fpn-norm gn'),
    Extension('cascade', add_cascade_flags, _cascade_settings_of, is_on=lambda s: bool(s['cascade_ious']), off=NO_CASCADE, state_key='cascade',
              switch='--cascade 1', model_noun='a cascade model', settings_noun='the cascade', refuses_tta=True),
    Extension('mask_iou', add_mask_iou_flags, lambda a, training: mask_iou_settings(a.mask_iou, a.mask_iou_weight if training else None, a.head_arch),
              is_on=lambda s: s['mask_iou'], weight_flag='--mask-iou-weight', off=NO_MASK_IOU, state_key='mask_iou',
              switch='--mask-iou 1', model_noun='a Mask Scoring model', settings_noun='the Mask Scoring settings', refuses_tta=True,
              mask_heads_only=(lambda a: a.mask_iou or a.mask_iou_weight is not None,
                               '--mask-iou scores binary masks: it is defined for mask heads, not for keypoint training (train_keypoints.py)'),
              model_kwargs=lambda s: {'mask_iou': s['mask_iou']}, chain_keys=('mask_iou_weight',), loss_key='maskiou_loss'),
    Extension('point_rend', add_point_rend_flags, lambda a, training: point_rend_flag_settings(a, a.head_arch, a.mask_iou, weight=training),
              is_on=lambda s: s['point_rend'], weight_flag='--point-loss-weight', off=NO_POINT_REND, state_key='point_rend',
              switch='--point-rend 1', model_noun='a PointRend model', settings_noun='the PointRend settings', refuses_tta=True,
              mask_heads_only=(lambda a: a.point_rend,
                               '--point-rend refines binary masks: it is defined for mask heads, not for keypoint training (train_keypoints.py)'),
              model_kwargs=point_rend_model_kwargs, chain_keys=('point_loss_weight',), loss_key='point_loss'))
# how each script's refusal spells its test-time augmentation flags
TTA_FLAGS = {'--tta-': '--tta-sizes / --tta-hflip', '--eval-tta-': '--eval-tta-*'}


def add_extension_flags(parser, both=lambda name: (name,), training=False):
    """The flags of every extension (train_keypoints.py takes both spellings through ``both``); the weight flags with ``training`` only."""
    for e in EXTENSIONS:
        e.add_flags(parser, both, **({'weight': training} if e.weight_flag else {}))


def extension_settings(args, tta_prefix='--tta-', training=False, keypoints=False):
    """{name: settings} of every extension from the parsed flags, checked before the model is built.  ValueError, extension by extension: for
    keypoint training of a mask-heads-only one, for what its settings refuse, and for test-time augmentation (the flags ``tta_prefix``sizes /
    hflip: '--tta-' in evaluate.py and demo.py, '--eval-tta-' in train.py) on top of one MaskRCNN.use_test_augmentation refuses."""
    tta = tta_prefix.strip('-').replace('-', '_') + '_'
    tta = getattr(args, tta + 'sizes') or getattr(args, tta + 'hflip')
    out = {}
    for e in EXTENSIONS:
        if keypoints and e.mask_heads_only and e.mask_heads_only[0](args):
            raise ValueError(e.mask_heads_only[1])
        out[e.name] = e.settings(args, training)
        if tta and e.refuses_tta and e.is_on(out[e.name]):
            raise ValueError('%s does not go with %s: test-time augmentation of %s is not supported' % (e.switch, TTA_FLAGS[tta_prefix], e.model_noun))
    return out


def model_kwargs(settings, keypoints=False):
    """The MaskRCNN keyword arguments of extension_settings' result (a keypoint model takes none from the mask-heads-only extensions)."""
    out = {}
    for e in EXTENSIONS:
        if not (keypoints and e.mask_heads_only):
            out.update(e.model_kwargs(settings[e.name]))
    return out


def chain_kwargs(settings):
    """The FPNMaskRCNNTrainChain keyword arguments of extension_settings' result, for a mask model."""
    return {k: settings[e.name][k] for e in EXTENSIONS for k in e.chain_keys}


def state_records(settings):
    """What trainer_<it>.pt records of extension_settings' result: {state key: settings}."""
    return {e.state_key: settings[e.name] for e in EXTENSIONS if e.state_key}


def check_resume(resume, key, off_record, now, noun, path=''):
    """A resumed run has the settings its checkpoint recorded under ``key`` (a state without the key: ``off_record``): the flat parameter and
    momentum buffers, the data order and the schedule follow from them."""
    was = resume.get(key, off_record)
    if was != now:
        raise ValueError('--resume %s: the checkpoint was trained with %s %r, this run asks for %r' % (path, noun, was, now))


# ---- labels and the model -----------------------------------------------------------------------------------------------------------------
def read_labels(label_file):
    """The category names of --label_file (None when the file does not exist: every category)."""
    if not os.path.exists(label_file):
        return None
    with open(label_file) as f:
        return f.read().strip().split('\n')


def use_score_preset(model, preset, score_thresh=None):
    """``preset`` ('visualize' / 'evaluate') on the model, its score threshold overridden by --score-thresh when given."""
    model.use_preset(preset)
    if score_thresh is not None:
        model.score_thresh = score_thresh


def build_inference_model(args, preset=None):
    """MaskRCNN of the flags --gpu / --backbone / --head-arch / --head-norm / --fpn-norm / --gn-groups / --cascade* / --mask-iou / --point-rend* / --dcn-* / --label_file with --weight loaded (keys missing from the file keep their
    initial values) and, when ``preset`` is given, use_score_preset(model, preset, --score-thresh).  A keypoint head is COCO's: one class,
    17 keypoints; a mask head has one class per label (80 without a label file)."""
    import torch
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.utils import chainer_npz
    extensions = model_kwargs(extension_settings(args))
    extensions.update(dcn_model_kwargs(dcn_settings_of(args)))
    dev =torch.device('cuda', args.gpu)
    torch.cuda.set_device(dev)
    if args.head_arch == 'fpn_keypoint':
        model = MaskRCNN(n_fg_class=1, n_keypoints=17, backbone=args.backbone, head_arch=args.head_arch, device=dev, **extensions)
    else:
        labels = read_labels(args.label_file)
        model = MaskRCNN(n_fg_class=len(labels) if labels else 80, backbone=args.backbone, head_arch=args.head_arch, device=dev, **extensions)
    if args.weight:
        if not os.path.exists(args.weight):
            raise FileNotFoundError('--weight %s does not exist' % args.weight)
        chainer_npz.load_npz(args.weight, model, strict=False)
    if preset is not None:
        use_score_preset(model, preset, args.score_thresh)
    return model
