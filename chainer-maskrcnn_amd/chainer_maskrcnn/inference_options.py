"""The inference options of the entry scripts, stated once: the test-time augmentation and box post-processing flags of evaluate.py and
demo.py (train.py declares them with the prefix '--eval-' for its periodic evaluator), what they turn into on a model, the label file and
the model a checkpoint is scored or drawn with.  Importing this module needs neither a device nor the training script."""
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


def check_cascade_flags(args, tta_prefix='--'):
    """The cascade flags of an inference script (evaluate.py, demo.py) checked before the model is built: cascade_flag_settings' refusals, and
    no test-time augmentation on top of a cascade (MaskRCNN.use_test_augmentation refuses it)."""
    settings = cascade_flag_settings(args.cascade, args.cascade_ious, args.cascade_stds, args.head_arch, args.backbone)
    if settings['cascade_ious'] and (args.tta_sizes or args.tta_hflip):
        raise ValueError('--cascade 1 does not go with %stta-sizes / %stta-hflip: test-time augmentation of a cascade model is not supported'
                         % (tta_prefix, tta_prefix))
    return settings


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


def check_mask_iou_flags(args, tta_prefix='--'):
    """--mask-iou of an inference script (evaluate.py, demo.py) checked before the model is built: mask_iou_settings' refusals, and no
    test-time augmentation on top of it (MaskRCNN.use_test_augmentation refuses it)."""
    settings = mask_iou_settings(args.mask_iou, None, args.head_arch)
    if settings['mask_iou'] and (args.tta_sizes or args.tta_hflip):
        raise ValueError('--mask-iou 1 does not go with %stta-sizes / %stta-hflip: test-time augmentation of a Mask Scoring model is not '
                         'supported' % (tta_prefix, tta_prefix))
    return settings


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


def check_point_rend_flags(args, tta_prefix='--'):
    """--point-rend of an inference script (evaluate.py, demo.py) checked before the model is built: point_rend_flag_settings' refusals,
    and no test-time augmentation on top of it (MaskRCNN.use_test_augmentation refuses it)."""
    settings = point_rend_flag_settings(args, args.head_arch, getattr(args, 'mask_iou', 0))
    if settings['point_rend'] and (args.tta_sizes or args.tta_hflip):
        raise ValueError('--point-rend 1 does not go with %stta-sizes / %stta-hflip: test-time augmentation of a PointRend model is not '
                         'supported' % (tta_prefix, tta_prefix))
    return settings


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
    """MaskRCNN of the flags --gpu / --backbone / --head-arch / --head-norm / --fpn-norm / --gn-groups / --cascade* / --mask-iou / --point-rend* / --label_file with --weight loaded (keys missing from the file keep their
    initial values) and, when ``preset`` is given, use_score_preset(model, preset, --score-thresh).  A keypoint head is COCO's: one class,
    17 keypoints; a mask head has one class per label (80 without a label file)."""
    import torch
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.utils import chainer_npz
    norm = head_norm_settings(args.head_norm, args.gn_groups, args.head_arch)
    norm.update(fpn_norm_settings(getattr(args, 'fpn_norm', 'none'), args.gn_groups, args.backbone))
    norm.update(cascade_flag_settings(args.cascade, args.cascade_ious, args.cascade_stds, args.head_arch, args.backbone))
    norm['mask_iou'] = mask_iou_settings(getattr(args, 'mask_iou', 0), None, args.head_arch)['mask_iou']
    norm.update(point_rend_model_kwargs(point_rend_flag_settings(args, args.head_arch, norm['mask_iou'])))
    dev =torch.device('cuda', args.gpu)
    torch.cuda.set_device(dev)
    if args.head_arch == 'fpn_keypoint':
        model = MaskRCNN(n_fg_class=1, n_keypoints=17, backbone=args.backbone, head_arch=args.head_arch, device=dev, **norm)
    else:
        labels = read_labels(args.label_file)
        model = MaskRCNN(n_fg_class=len(labels) if labels else 80, backbone=args.backbone, head_arch=args.head_arch, device=dev, **norm)
    if args.weight:
        if not os.path.exists(args.weight):
            raise FileNotFoundError('--weight %s does not exist' % args.weight)
        chainer_npz.load_npz(args.weight, model, strict=False)
    if preset is not None:
        use_score_preset(model, preset, args.score_thresh)
    return model
