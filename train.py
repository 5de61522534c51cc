#!/usr/bin/env python3
"""Training entry point with the flags, constants and log keys of the reference's train.py (:62-74 flags, :95-98
model, :107-109 optimizer, :117-132 updater wiring, :134-161 snapshot / LR shift / log), on the MI355X-native path.

The reference's train.py imports chainer / chainercv / chainerui / cv2 / pycocotools (train.py:1-8), none of which
exist on the target machine, so this is the repo's own counterpart: same CLI, JSON-lines log in --out.  Data:
synthetic COCO-shaped batches (--synthetic 1, the default - the box has no dataset), or real COCO through
chainer_maskrcnn/dataset (--synthetic 0 --anno-dir data/annotations --img-dir data --data-type 2017: the
reference's COCOMaskLoader / COCOKeypointsLoader + Transform, a prefetching loader, no pycocotools / cv2).
Multi GPU: launch with `python -m torch.distributed.run --nproc-per-node N train.py --multi-gpu 1 ...`
(one process per GPU, RCCL all-reduce of the flat gradient buffer; the reference forks 8 workers itself).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'chainer-maskrcnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chainer_maskrcnn.inference_options import (DCN_NOUN, EXTENSIONS, NO_DCN, add_boundary_flag, add_boxpost_flags, add_dcn_flags, add_extension_flags, add_tta_flags, boundary_iou_types, boxpost_settings, chain_kwargs,  # noqa: E402
                                                check_resume, dcn_model_kwargs, dcn_settings_of, extension_settings, model_kwargs, read_labels, state_records, tta_settings, use_boxpost,
                                                use_tta)
from chainer_maskrcnn.utils.chainer_npz import load_npz, save_npz  # noqa: E402  (load_npz: strict=False, like train.py:99-101)

SYNTHETIC_VAL_IMAGES = 16           # the synthetic "val split" of --synthetic 1 --eval-images 0
AUGMENT_SEED = 5678                 # seed of the per-example augmentation decisions (dataset/augment.py), recorded in trainer_<it>.pt
NO_FREEZE = {'bn': 0, 'at': 0}       # what a trainer state without the 'freeze' key was trained with
NO_OPTIM = {'accum_steps': 1, 'grad_clip': 0.0, 'schedule': None}      # what a trainer state without the 'optim' key was trained with
NO_AUGMENT = {'hflip': 0, 'min_sizes': None, 'seed': AUGMENT_SEED}     # what a trainer state without the 'augment' key was trained with
# what a resumed run must repeat of its trainer_<it>.pt, in the order it is checked: (key, a state without the key, the noun of the refusal)
RESUME_CHECKS = ((('augment', NO_AUGMENT, 'augmentation'),) + tuple((e.state_key, e.off, e.settings_noun) for e in EXTENSIONS if e.state_key)
                 + (('dcn', NO_DCN, DCN_NOUN), ('freeze', NO_FREEZE, 'freezing'), ('optim', NO_OPTIM, 'the optimizer recipe')))


def build_parser(keypoints=False):
    parser = argparse.ArgumentParser(description='Mask R-CNN')
    parser.add_argument('--gpu', '-g', type=int, default=0)
    parser.add_argument('--lr', '-l', type=float, default=1e-3)
    parser.add_argument('--out', '-o', default='result', help='Output directory')
    parser.add_argument('--iteration', '-i', type=int, default=200000)
    parser.add_argument('--weight', '-w', type=str, default='')
    parser.add_argument('--resnet50-npz', type=str, default='', help="a chainer.links.ResNet50Layers snapshot for the bottom-up pathway (what ResNet50Layers('auto') loads in the reference, feature_pyramid_network.py:22)")
    if keypoints:   # train_keypoints.py spells its flags with underscores (train_keypoints.py:73-89)
        parser.add_argument('--label_file', '-f', type=str, default='data/label_coco.txt')      # (:79-80; unused there too: n_fg_class is 1)
        parser.add_argument('--backbone', type=str, default='fpn')
        parser.add_argument('--head_arch', '-a', type=str, default='fpn_keypoint')
        parser.add_argument('--multi_gpu', '-m', type=int, default=0)
        parser.add_argument('--batch_size', '-b', type=int, default=1)
        parser.add_argument('--dataset', default='coco', choices=['coco', 'depth'])               # :86
        parser.add_argument('--n_mask_convs', type=int, default=None)                             # :87 (None: the model's 8, maskrcnn.py:110-111)
        parser.add_argument('--min_size', type=int, default=600)                                  # :88
        parser.add_argument('--max_size', type=int, default=1000)                                 # :89
        parser.add_argument('--depth-list', default='data/rgbd/train.txt', help='--dataset depth: the list file (train_keypoints.py:105)')
        parser.add_argument('--depth-root', default='data/rgbd/', help='--dataset depth: directory the listed .npz paths are relative to')
    else:
        parser.add_argument('--label_file', '-f', type=str, default='data/label_coco.txt')
        parser.add_argument('--backbone', type=str, default='fpn')
        parser.add_argument('--head-arch', '-a', type=str, default='fpn')
        parser.add_argument('--multi-gpu', '-m', type=int, default=0)
        parser.add_argument('--batch-size', '-b', type=int, default=1)
    parser.add_argument('--synthetic', type=int, default=1, help='1: synthetic COCO-shaped batches; 0: COCO from --anno-dir / --img-dir')
    parser.add_argument('--anno-dir', default='data/annotations')
    parser.add_argument('--img-dir', default='data')
    parser.add_argument('--data-type', default='2017')
    parser.add_argument('--num-workers', type=int, default=8, help='decode / transform threads of the COCO loader')
    parser.add_argument('--max-gt', type=int, default=0, help='instances kept per image (0: all; static shapes when > 0)')
    parser.add_argument('--image-size', type=int, nargs=2, default=[800, 800])
    parser.add_argument('--gemm-arithmetic', default='bf16x6_behind_backbone', choices=['f32', 'bf16x6_behind_backbone', 'bf16x6_backward', 'bf16x6'],
                        help='arithmetic of the convolution GEMMs (model/fpn_maskrcnn_train_chain.py GEMM_ARITHMETIC): float32 tensors and float32 '
                             'accumulation in all three; bf16x6 = float32-accurate three-plane emulation on the bf16 MFMA')
    parser.add_argument('--log-interval', type=int, default=100)
    parser.add_argument('--snapshot-interval', type=int, default=5000)
    parser.add_argument('--lr-shift-interval', type=int, default=0, help='iterations between lr x0.1 (reference: 2 epochs)')
    parser.add_argument('--grad-average', type=int, default=0, help='multi GPU: 1 = average the gradients over the ranks (extension); '
                                                                   '0 = sum them with the un-scaled lr, as the reference does')
    parser.add_argument('--resume', default='', help='trainer_<iteration>.pt written next to the NPZ snapshots: parameters, momentum, '
                                                     'BN statistics, sampler seeds, iteration and lr - continues bit-identically')
    parser.add_argument('--profile', type=int, nargs=2, default=None, metavar=('FIRST', 'LAST'),
                        help='bracket iterations FIRST..LAST with roctx ranges (step / forward+backward / update) for '
                             '`rocprofv3 --marker-trace --kernel-trace -- python3 train.py ...`')
    parser.add_argument('--eval-interval', type=int, default=0,
                        help='iterations between validation mAP evaluations (InstanceSegmentationVOCEvaluator on the val split, '
                             'reference train.py:164-166 uses 10000); 0 = off')
    parser.add_argument('--eval-images', type=int, default=0,
                        help='images of the val split per evaluation (0: the whole split; --synthetic 1: %d images)' % SYNTHETIC_VAL_IMAGES)
    parser.add_argument('--eval-metric', default='mask_voc', choices=['mask_voc', 'mask_coco', 'keypoint_coco'],
                        help='metric of --eval-interval: mask_voc = PASCAL VOC mask mAP (mask heads, InstanceSegmentationVOCEvaluator); '
                             'mask_coco = COCO mask and box AP over IoU .50:.95 (mask heads, InstanceSegmentationCOCOEvaluator); '
                             'keypoint_coco = COCO keypoint AP over OKS .50:.95 (keypoint heads, KeypointCOCOEvaluator)')
    add_tta_flags(parser, '--eval-')
    add_boxpost_flags(parser, '--eval-')
    add_boundary_flag(parser, '--eval-')
    parser.add_argument('--hflip', type=int, default=0, choices=[0, 1],
                        help='1: mirror each training example with probability 0.5 (images, masks, boxes; keypoints with their left / right '
                             'channels swapped); --synthetic 0 only')
    parser.add_argument('--min-sizes', type=int, nargs='+', default=None, metavar='N',
                        help='scale jitter: each training example\'s short side is drawn uniformly from these sizes (the long side stays '
                             'capped by the model\'s max_size); --synthetic 0 only.  Default: the model\'s min_size')
    parser.add_argument('--freeze-bn', type=int, default=0, choices=[0, 1],
                        help='1: the ResNet\'s BatchNorm layers are frozen in the training step - running statistics, constant gamma / beta '
                             '(MaskRCNN.freeze); meant for a backbone imported with --resnet50-npz / --weight')
    parser.add_argument('--freeze-at', type=int, default=0, choices=[0, 1, 2, 3, 4, 5],
                        help='k: the stem and the stages res2 .. res{k} are not trained and take no backward pass (1: stem only, 2: the usual '
                             'fine-tuning recipe, 5: the whole ResNet); needs --freeze-bn 1')
    # train_keypoints.py spells its flags with underscores: it takes both spellings of these
    both = (lambda name: (name.replace('-', '_').replace('__', '--', 1), name)) if keypoints else (lambda name: (name,))
    parser.add_argument(*both('--accum-steps'), type=int, default=1, metavar='K',
                        help='gradient accumulation: one iteration stays one optimizer update and consumes K batches (K-1 x accumulate, then '
                             'update) - the step the reference takes with K workers of one batch each; images/sec counts all of them, the '
                             'logged losses are those of the iteration\'s LAST micro-batch; --grad-average 1 also averages over K')
    parser.add_argument(*both('--grad-clip'), type=float, default=0.0, metavar='T',
                        help='clip the gradient to global L2 norm T (optimizers.GradientClipping: the raw summed / averaged gradient, before '
                             'weight decay; a non-finite norm skips the update); logs main/grad_norm and skipped_updates.  0 = off')
    parser.add_argument(*both('--warmup-iterations'), type=int, default=0, metavar='W',
                        help='linear learning-rate warmup over the first W updates, from --warmup-factor x lr (optimizers.LRSchedule)')
    parser.add_argument(*both('--warmup-factor'), type=float, default=1.0 / 3, metavar='F')
    parser.add_argument(*both('--lr-steps'), type=int, nargs='+', default=None, metavar='S',
                        help='lr x0.1 behind each of these iterations (e.g. 60000 80000 of 90000); not together with --lr-shift-interval')
    parser.add_argument(*both('--lsj-size'), type=int, default=0, metavar='S',
                        help='large-scale jitter: every example is resized by a random factor (its longer side to S x a scale drawn from '
                             '--lsj-scale), cropped to at most S x S at a random position and padded to an S x S canvas - every batch has '
                             'that one shape; S a multiple of 64; --synthetic 0 only, not with --min-sizes.  0 = off')
    parser.add_argument(*both('--lsj-scale'), type=float, nargs=2, default=[0.1, 2.0], metavar=('LO', 'HI'),
                        help='the scale range of --lsj-size')
    parser.add_argument(*both('--copy-paste'), type=float, default=0.0, metavar='P',
                        help='Simple Copy-Paste on top of --lsj-size: with probability P an example receives a random half of the instances '
                             'of the next example of its batch, pasted over it (occluded masks are cut, boxes recomputed, covered instances '
                             'dropped); mask heads only, --batch-size >= 2, --synthetic 0.  0 = off')
    add_extension_flags(parser, both, training=True)
    add_dcn_flags(parser, both)
    parser.add_argument(*both('--box-loss'), default='smooth_l1', choices=['smooth_l1', 'giou', 'diou', 'ciou'],
                        help='box regression loss of the RoI head: smooth_l1 = the reference\'s, on the encoded deltas; giou / diou / ciou = on '
                             'the decoded box against the decoded target (FPNMaskRCNNTrainChain box_loss; same targets, normaliser and '
                             'checkpoints)')
    parser.add_argument(*both('--rpn-box-loss'), default='smooth_l1', choices=['smooth_l1', 'giou', 'diou', 'ciou'],
                        help='the same choice for the RPN, against the anchors')
    parser.add_argument(*both('--box-loss-weight'), type=float, default=1.0, metavar='W',
                        help='multiplies the --box-loss giou / diou / ciou value and gradient (smooth_l1 takes 1.0 only)')
    parser.add_argument(*both('--rpn-box-loss-weight'), type=float, default=1.0, metavar='W', help='the same for --rpn-box-loss')
    return parser


def optim_settings(args):
    """The optimizer-side recipe of a run as recorded in trainer_<it>.pt (NO_OPTIM when all off), with the LRSchedule it describes (or None);
    raises on a refused combination."""
    from chainer_maskrcnn.optimizers import LRSchedule
    k, clip, W = int(args.accum_steps), float(args.grad_clip), int(args.warmup_iterations)
    if k < 1:
        raise ValueError('--accum-steps must be at least 1, got %d' % k)
    if clip < 0 or clip != clip:
        raise ValueError('--grad-clip must be positive (0 = off), got %r' % clip)
    if W < 0:
        raise ValueError('--warmup-iterations must not be negative, got %d' % W)
    if args.lr_steps and args.lr_shift_interval:
        raise ValueError('--lr-steps and --lr-shift-interval both schedule the learning-rate drops: give one of them')
    schedule = None
    if args.lr_steps or W > 0:
        steps = args.lr_steps or ()
        if args.lr_shift_interval:      # warmup in front of the periodic x0.1: the same drops, as a function of the iteration
            steps = range(args.lr_shift_interval, args.iteration + 1, args.lr_shift_interval)
        schedule = LRSchedule(args.lr, W, args.warmup_factor, steps)
    return {'accum_steps': k, 'grad_clip': clip, 'schedule': None if schedule is None else schedule.describe()}, schedule


def freeze_settings(args):
    """The freezing of a run as recorded in trainer_<it>.pt (NO_FREEZE when off); raises on a combination MaskRCNN.freeze refuses."""
    bn, at = int(args.freeze_bn), int(args.freeze_at)
    if not 0 <= at <= 5:
        raise ValueError('--freeze-at must be in 0..5, got %d' % at)
    if bn not in (0, 1):
        raise ValueError('--freeze-bn must be 0 or 1, got %d' % bn)
    if at > 0 and not bn:
        raise ValueError('--freeze-at %d needs --freeze-bn 1 (a frozen prefix with batch-statistics BatchNorm is not implemented)' % at)
    return {'bn': bn, 'at': at}


def augment_settings(args):
    """The augmentation of a run as recorded in trainer_<it>.pt (NO_AUGMENT when off)."""
    settings = {'hflip': int(args.hflip), 'min_sizes': [int(s) for s in args.min_sizes] if args.min_sizes else None, 'seed': AUGMENT_SEED}
    if args.lsj_size:
        settings['lsj'] = {'size': int(args.lsj_size), 'scale': [float(v) for v in args.lsj_scale]}
    if args.copy_paste:
        settings['copy_paste'] = float(args.copy_paste)
    return settings


def _eval_boxpost_settings(args):
    """--eval-soft-nms / --eval-soft-nms-sigma / --eval-box-vote-thresh / --eval-max-detections: they act on the periodic evaluator's
    predictions, so they are refused without one."""
    b = boxpost_settings(args.eval_soft_nms, args.eval_soft_nms_sigma, args.eval_box_vote_thresh, args.eval_max_detections, '--eval-')
    if b is not None and args.eval_interval <= 0:
        raise ValueError('--eval-soft-nms / --eval-box-vote-thresh / --eval-max-detections change the predictions of the periodic '
                         'evaluator: they need --eval-interval > 0')
    return b


def _check_copy_paste_args(args, keypoints):
    p = args.copy_paste
    if not 0.0 < p <= 1.0:
        raise ValueError('--copy-paste: the probability must lie in (0, 1] (0 = off), got %r' % p)
    if keypoints:
        raise ValueError('--copy-paste pastes instance masks: it is defined for mask heads, not for keypoint data (train_keypoints.py)')
    if args.synthetic:
        raise ValueError('--copy-paste augments the dataset loader (--synthetic 0); the synthetic batches (--synthetic 1) are not augmented')
    if not args.lsj_size:
        raise ValueError('--copy-paste composes two large-scale-jittered canvases: it needs --lsj-size')
    if args.batch_size < 2:
        raise ValueError('--copy-paste pastes from the next example of the batch: it needs --batch-size >= 2, got %d' % args.batch_size)


def _check_augment_args(args, keypoints=False):
    if args.copy_paste:
        _check_copy_paste_args(args, keypoints)
    if (args.hflip or args.min_sizes) and args.synthetic:
        raise ValueError('--hflip / --min-sizes augment the dataset loader (--synthetic 0); the synthetic batches (--synthetic 1) are not '
                         'augmented')
    if args.min_sizes and any(s <= 0 for s in args.min_sizes):
        raise ValueError('--min-sizes: every size must be positive, got %s' % args.min_sizes)
    if not args.lsj_size:
        return
    lo, hi = args.lsj_scale
    if args.lsj_size < 0 or args.lsj_size % 64:
        raise ValueError('--lsj-size must be a positive multiple of 64 (the coarsest pyramid stride), got %d' % args.lsj_size)
    if not lo > 0:
        raise ValueError('--lsj-scale: LO must be positive, got %r' % lo)
    if lo > hi:
        raise ValueError('--lsj-scale: LO must not exceed HI, got %r > %r' % (lo, hi))
    if args.synthetic:
        raise ValueError('--lsj-size augments the dataset loader (--synthetic 0); the synthetic batches (--synthetic 1) are not augmented')
    if args.min_sizes:
        raise ValueError('--min-sizes and --lsj-size are two different resize rules: give one of them')
    if getattr(args, 'dataset', 'coco') == 'depth':
        raise ValueError('--lsj-size: --dataset depth is transformed on the host only and has no large-scale jitter')


def _keypoint_names(args, data):
    """The keypoint names of a keypoint dataset: COCO's from the annotation file's person category (COCO's 17 names when the file has
    none), the depth dataset's 20 joints."""
    from chainer_maskrcnn.dataset import augment
    if args.dataset == 'depth':
        return augment.DEPTH_KEYPOINT_NAMES
    return data.coco.cats.get(1, {}).get('keypoints') or augment.COCO_KEYPOINT_NAMES


def _keypoint_flip_perm(args, data):
    """The flip map of a keypoint dataset's names.  ValueError when the names do not pair completely."""
    from chainer_maskrcnn.dataset import augment
    names = _keypoint_names(args, data)
    if len(names) != data.n_keypoints:
        raise ValueError('--hflip 1: %d keypoint names for %d keypoints' % (len(names), data.n_keypoints))
    try:
        return augment.flip_permutation(names)
    except ValueError as e:
        raise ValueError('--hflip 1: this keypoint dataset has no complete left / right flip map (%s)' % e)


def run(args, keypoints=False):
    from chainer_maskrcnn.model.maskrcnn import MaskRCNN
    from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, box_loss_settings, calc_mask_loss, calc_keypoint_loss
    from chainer_maskrcnn.optimizers import MomentumSGD, WeightDecay, GradientClipping
    from chainer_maskrcnn.utils.synthetic import make_batch
    world = int(os.environ.get('WORLD_SIZE', 1))
    rank = int(os.environ.get('RANK', 0))
    if args.eval_interval > 0 and keypoints and args.eval_metric != 'keypoint_coco':
        raise ValueError('--eval-interval: validation mAP (--eval-metric %s) is computed for mask heads only; keypoint runs take '
                         '--eval-metric keypoint_coco' % args.eval_metric)
    if args.eval_metric == 'keypoint_coco' and not keypoints:
        raise ValueError('--eval-metric keypoint_coco: COCO keypoint AP needs a keypoint head (train_keypoints.py); mask heads take mask_voc '
                         'or mask_coco')
    if args.eval_metric == 'keypoint_coco' and getattr(args, 'dataset', 'coco') == 'depth':
        raise ValueError('--eval-metric keypoint_coco: COCO defines OKS sigmas for its 17 keypoints only; --dataset depth has 20')
    if args.eval_interval > 0 and world > 1:
        raise ValueError('--eval-interval: evaluation runs in single-process training only; with %d ranks it is not supported '
                         '(the reference\'s multi-GPU branch has no test iterator either, train.py:117-121, and would fail there)' % world)
    _check_augment_args(args, keypoints)
    boundary_iou_types(args.eval_boundary, args.eval_metric, keypoints, '--eval-')
    if args.eval_boundary and args.eval_interval <= 0:
        raise ValueError('--eval-boundary 1 adds a metric to the periodic evaluator: it needs --eval-interval > 0')
    eval_boxpost = _eval_boxpost_settings(args)
    resume = torch.load(args.resume, map_location='cpu', weights_only=False) if args.resume else None
    extensions = extension_settings(args, '--eval-tta-', training=True, keypoints=keypoints)
    dcn = dcn_settings_of(args)
    box_loss = box_loss_settings(args.box_loss, args.rpn_box_loss, args.box_loss_weight, args.rpn_box_loss_weight)
    freeze = freeze_settings(args)
    optim, schedule = optim_settings(args)
    recorded = dict({'augment': augment_settings(args), 'dcn': dcn, 'freeze': freeze, 'optim': optim}, **state_records(extensions))     # of trainer_<it>.pt
    if resume is not None:
        for key, off_record, noun in RESUME_CHECKS:
            check_resume(resume, key, off_record, recorded[key], noun, args.resume)
    accum = optim['accum_steps']
    if freeze['bn'] and not (args.weight or args.resnet50_npz or args.resume) and rank == 0:
        print('warning: --freeze-bn 1 without --weight / --resnet50-npz / --resume freezes freshly initialised BatchNorm statistics '
              '(mean 0, variance 1)')
    data = None
    if not args.synthetic:          # the training set (before any device work: a keypoint set's flip map is checked here)
        from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader, COCOKeypointsLoader
        if keypoints and args.dataset == 'depth':
            from chainer_maskrcnn.dataset.depth_dataset import DepthDataset
            data = DepthDataset(path=args.depth_list, root=args.depth_root)
        elif keypoints:
            data = COCOKeypointsLoader(anno_dir=args.anno_dir, img_dir=args.img_dir, data_type=args.data_type)
        else:
            data = COCOMaskLoader(anno_dir=args.anno_dir, img_dir=args.img_dir, data_type=args.data_type,
                                  category_filter=read_labels(args.label_file))
    augment = None
    if args.hflip or args.min_sizes or args.lsj_size:
        from chainer_maskrcnn.dataset.augment import Augment
        augment = Augment(hflip_prob=0.5 if args.hflip else 0.0, min_sizes=args.min_sizes, seed=AUGMENT_SEED,
                          keypoint_perm=_keypoint_flip_perm(args, data) if keypoints and args.hflip else None,
                          lsj_size=args.lsj_size or None, lsj_scale=args.lsj_scale, copy_paste_prob=args.copy_paste)
    local = int(os.environ.get('LOCAL_RANK', args.gpu))
    ndev = max(1, torch.cuda.device_count())
    lws = int(os.environ.get('LOCAL_WORLD_SIZE', 1))
    if lws > ndev and ndev != 1:        # (ndev == 1: a launcher that shows every rank only its own GPU)
        raise SystemExit('train.py: %d local ranks but %d visible GPUs - one process per GPU is required' % (lws, ndev))
    dev = torch.device('cuda', local % ndev if 'LOCAL_RANK' in os.environ else local)
    if world > 1:       # one process per GPU: host threads (enqueue loop, loader workers, RCCL proxy) on the GPU's NUMA node
        from chainer_maskrcnn.utils.affinity import pin_rank
        cpus = pin_rank(local, int(os.environ.get('LOCAL_WORLD_SIZE', world)))
        if cpus:
            print('rank %d: pinned to %d cores (%d..%d)' % (rank, len(cpus), cpus[0], cpus[-1]))
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        from chainer_maskrcnn.optimizers import init_process_group
        init_process_group('nccl')
    if keypoints:
        n_fg, K = 1, 20 if args.dataset == 'depth' else 17          # DepthDataset.n_keypoints / COCOKeypointsLoader.n_keypoints
        labels = None
        faster_rcnn = MaskRCNN(n_fg_class=n_fg, n_keypoints=K, backbone=args.backbone, head_arch=args.head_arch, n_mask_convs=args.n_mask_convs,
                               min_size=args.min_size, max_size=args.max_size, device=dev, **model_kwargs(extensions, keypoints=True),
                               **dcn_model_kwargs(dcn))
        loss_fun = calc_keypoint_loss
        if K != 17:         # train_keypoints.py:122: lambda x, y, z, w: calc_mask_loss(x, y, z, w, num_keypoints=n_keypoints)
            loss_fun = lambda x, y, z, w: calc_keypoint_loss(x, y, z, w, num_keypoints=K)
            loss_fun.fused_kind = calc_keypoint_loss.fused_kind
        model = FPNMaskRCNNTrainChain(faster_rcnn, mask_loss_fun=loss_fun, binary_mask=False, gemm_arithmetic=args.gemm_arithmetic, **box_loss)
    else:
        labels = read_labels(args.label_file)
        n_fg, K = len(labels) if labels else 80, None
        faster_rcnn = MaskRCNN(n_fg_class=n_fg, backbone=args.backbone, head_arch=args.head_arch, device=dev, **model_kwargs(extensions),
                               **dcn_model_kwargs(dcn))
        model = FPNMaskRCNNTrainChain(faster_rcnn, mask_loss_fun=calc_mask_loss, gemm_arithmetic=args.gemm_arithmetic, **chain_kwargs(extensions),
                                      **box_loss)
    faster_rcnn.use_preset('evaluate')
    if args.resnet50_npz:           # ImageNet initialisation of the bottom-up pathway (before --weight, which may override it)
        from chainer_maskrcnn.utils import chainer_npz
        n = len(chainer_npz.load_resnet50_npz(args.resnet50_npz, faster_rcnn))
        if rank == 0:
            print('ResNet-50 snapshot: %d arrays loaded from %s' % (n, args.resnet50_npz))
    if args.weight and os.path.exists(args.weight):
        load_npz(args.weight, faster_rcnn)
    if freeze != NO_FREEZE:
        faster_rcnn.freeze(bn=bool(freeze['bn']), at=freeze['at'])
    optimizer = MomentumSGD(lr=args.lr, momentum=0.9, average_accumulated=bool(args.grad_average))
    optimizer.setup(model)
    optimizer.add_hook(WeightDecay(rate=0.0005))
    if optim['grad_clip'] > 0:
        optimizer.add_hook(GradientClipping(optim['grad_clip']))
    if world > 1:
        optimizer.enable_data_parallel(average=bool(args.grad_average))
    bs = args.batch_size
    H, W = args.image_size
    os.makedirs(args.out, exist_ok=True)
    log = open(os.path.join(args.out, 'log'), 'a') if rank == 0 else None
    keys = ('loss', 'rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'mask_loss')
    keys += tuple(e.loss_key for e in EXTENSIONS if e.loss_key and e.is_on(extensions[e.name]))
    acc ={k: 0.0 for k in keys}
    loader = None
    if not args.synthetic:          # train.py:111-126: COCOMaskLoader(category_filter=labels, data_type='2017') + Transform
        from chainer_maskrcnn.dataset.transforms import RawTransform
        from chainer_maskrcnn.dataset.loader import BatchLoader
        if keypoints and args.dataset == 'depth':       # train_keypoints.py:103-109, 135: DepthDataset -> DepthTransformer -> Transform, on the host
            from chainer_maskrcnn.dataset.depth_dataset import DepthTransformer
            from chainer_maskrcnn.dataset.transforms import KeypointTransform
            jitter, kt = DepthTransformer(np.random.RandomState(4321 + rank)), KeypointTransform(faster_rcnn)
            tf = lambda ex, aug=None: kt(jitter(ex), aug)
        elif keypoints:
            tf = RawTransform(faster_rcnn, keypoints=True)      # host decodes, the GPU resizes (dataset/loader.py)
        else:
            tf = RawTransform(faster_rcnn)
        loader = BatchLoader(data, tf, batch_size=bs, shuffle=True, seed=1234, rank=rank, world=world,
                             num_workers=args.num_workers, max_gt=args.max_gt or None, keypoints=keypoints, device=dev,
                             start_ticket=_rank_ticket(resume['loader_ticket'], rank) if resume else 0, augment=augment)
    pool = []
    if loader is None:
        for j in range(8):
            b = make_batch((j + 1) * world + rank, bs, H, W, G=8, n_fg_class=n_fg, n_keypoints=K)
            pool.append([torch.from_numpy(b[k]).to(dev) for k in ('imgs', 'bboxes', 'labels', 'keypoints' if keypoints else 'masks')])
    first_it = 1
    if resume is not None:
        optimizer.load_state_dict(resume['optimizer'])
        first_it = resume['iteration'] + 1
    evaluator = _make_evaluator(args, faster_rcnn, labels, n_fg, K) if args.eval_interval > 0 else None
    if evaluator is not None:
        _use_eval_tta(args, faster_rcnn, evaluator)
        use_boxpost(faster_rcnn, eval_boxpost)
    rtx = _Roctx() if args.profile else None
    t0 = time.time()
    t_eval = 0.0            # seconds spent in evaluation: not part of the training throughput
    def next_batch(micro):
        if loader is not None:
            b = next(loader)
            # every image keeps its own resize factor and its own size inside the padded batch (the reference runs batch 1
            # per process, so its img_size / scale are always those of THE image: fpn_maskrcnn_train_chain.py:60-70)
            return [b[k] for k in ('imgs', 'bboxes', 'labels', 'keypoints' if keypoints else 'masks')], b['scales'], b['sizes']
        # a small pool of device-resident synthetic batches, cycled (generating one per step is host-bound)
        return pool[micro % len(pool)], 1.0, None

    for it in range(first_it, args.iteration + 1):
        if schedule is not None:
            optimizer.lr = schedule.lr_at(it)
        for j in range(accum - 1):      # --accum-steps: all but the last micro-batch of this update
            batch, scale, sizes = next_batch((it - 1) * accum + j + 1)
            optimizer.accumulate(model, *batch, scale, img_sizes=sizes)
        batch, scale, sizes = next_batch(it * accum)
        if rtx is not None and args.profile[0] <= it <= args.profile[1] and accum > 1:
            with rtx.range('step %d' % it):         # (an update() without the loss function would apply the accumulator alone)
                optimizer.update(model, *batch, scale, img_sizes=sizes)
        elif rtx is not None and args.profile[0] <= it <= args.profile[1]:
            with rtx.range('step %d' % it):
                with rtx.range('forward+backward'):
                    if optimizer.sync is not None:
                        optimizer.sync.begin()
                    loss = model(*batch, scale, img_sizes=sizes)
                    model.unit_upstream = True
                    try:
                        loss.backward()
                    finally:
                        model.unit_upstream = False
                with rtx.range('all-reduce wait + sgd'):
                    optimizer.update()
        else:
            optimizer.update(model, *batch, scale, img_sizes=sizes)
        validation = None
        if evaluator is not None and it % args.eval_interval == 0:       # after the update of this iteration, like a trainer extension
            te = time.time()
            validation = {'validation/' + k: v for k, v in evaluator.evaluate().items()}
            t_eval += time.time() - te
        if it % args.log_interval == 0 or it == args.iteration or validation is not None:       # one device->host sync per log interval
            obs = {k: float(v) for k, v in model.observation.items()}
            # (with --grad-clip an update whose gradient is not finite has been skipped on the device: logged, not fatal)
            if any(not np.isfinite(v) for v in obs.values()) and not optim['grad_clip'] > 0:
                raise FloatingPointError('non-finite loss at iteration %d: %r' % (it, obs))
            entry = {'iteration': it, 'lr': optimizer.lr, 'elapsed_time': time.time() - t0,
                     'images/sec': (it - first_it + 1) * accum * bs * world / (time.time() - t0 - t_eval)}
            entry.update({'main/' + k: v for k, v in obs.items()})
            if optim['grad_clip'] > 0:
                entry['main/grad_norm'] = float(optimizer.grad_norm)
                if int(optimizer.skipped_updates):
                    entry['skipped_updates'] = int(optimizer.skipped_updates)
            if validation is not None:
                entry.update(validation)
            if rank == 0:
                log.write(json.dumps(entry) + '\n')
                log.flush()
                print(entry)
        if args.lr_shift_interval and it % args.lr_shift_interval == 0:
            optimizer.lr *= 0.1                                       # ExponentialShift('lr', 0.1), train.py:139-140
        if it % args.snapshot_interval == 0:
            # every rank's data position goes into the trainer state: tickets count popped examples (skipped empty ones
            # included), so ranks can stand at different positions of their shards - a resumed rank continues from ITS own
            tickets = _all_rank_tickets(loader.ticket if loader is not None else 0, world, dev)
            if rank == 0:
                save_npz(os.path.join(args.out, 'model_%d.npz' % it), faster_rcnn)      # snapshot_object, train.py:134-137
                torch.save(dict({'iteration': it, 'optimizer': optimizer.state_dict(), 'loader_ticket': tickets}, **recorded),
                           os.path.join(args.out, 'trainer_%d.pt' % it))
    if loader is not None:
        loader.close()
    if world > 1:
        torch.distributed.destroy_process_group()


def _use_eval_tta(args, faster_rcnn, evaluator):
    """--eval-tta-*: test-time augmentation of the periodic evaluator's predictions.  A keypoint model's flip map comes from the val data's
    names (_keypoint_names; COCO's 17 names for the synthetic split)."""
    names = None
    data = getattr(evaluator.dataset, 'loader', None)
    if faster_rcnn.head_arch == 'fpn_keypoint' and not args.synthetic and data is not None:
        names = _keypoint_names(args, data)
    use_tta(faster_rcnn, tta_settings(args.eval_tta_sizes, args.eval_tta_hflip, args.eval_tta_max_size, faster_rcnn.min_size), names, '--eval-')


def _make_evaluator(args, faster_rcnn, labels, n_fg, K=None):
    """The val split of the run (reference train.py:113-115: COCOMaskLoader(split='val') + EvaluatorTransform) and its
    InstanceSegmentationVOCEvaluator; with --eval-metric mask_coco, every image of the val annotation file (COCOInstanceEvalDataset) and
    InstanceSegmentationCOCOEvaluator; with --eval-metric keypoint_coco, COCOKeypointsLoader(split='val') and KeypointCOCOEvaluator.
    --synthetic 1: deterministic make_batch images from seeds the training pool never uses."""
    from chainer_maskrcnn.evaluator import InstanceSegmentationVOCEvaluator, SyntheticEvalDataset, TransformedDataset, coco_mask_example
    if args.eval_metric == 'keypoint_coco':
        from chainer_maskrcnn.evaluator import COCOKeypointEvalDataset, KeypointCOCOEvaluator, SyntheticKeypointEvalDataset
        if args.synthetic:
            H, W = args.image_size
            data = SyntheticKeypointEvalDataset(args.eval_images or SYNTHETIC_VAL_IMAGES, H, W, n_keypoints=K)
        else:
            from chainer_maskrcnn.dataset.coco_dataset import COCOKeypointsLoader
            val = COCOKeypointsLoader(anno_dir=args.anno_dir, img_dir=args.img_dir, split='val', data_type=args.data_type)
            data = COCOKeypointEvalDataset(val, n=args.eval_images or None)
        return KeypointCOCOEvaluator(data, faster_rcnn)
    if args.eval_metric == 'mask_coco':
        from chainer_maskrcnn.evaluator import InstanceSegmentationCOCOEvaluator, SyntheticCOCOEvalDataset
        if args.synthetic:
            H, W = args.image_size
            data = SyntheticCOCOEvalDataset(args.eval_images or SYNTHETIC_VAL_IMAGES, H, W, n_fg_class=n_fg)
        else:
            from chainer_maskrcnn.dataset.coco_dataset import COCOInstanceEvalDataset
            data = COCOInstanceEvalDataset(anno_dir=args.anno_dir, img_dir=args.img_dir, split='val', data_type=args.data_type,
                                           category_filter=labels, n=args.eval_images or None)
        return InstanceSegmentationCOCOEvaluator(data, faster_rcnn, label_names=getattr(data, 'label_names', None) or labels,
                                                 iou_types=boundary_iou_types(args.eval_boundary, args.eval_metric, prefix='--eval-'))
    if args.synthetic:
        H, W = args.image_size
        data = SyntheticEvalDataset(args.eval_images or SYNTHETIC_VAL_IMAGES, H, W, n_fg_class=n_fg)
    else:
        from chainer_maskrcnn.dataset.coco_dataset import COCOMaskLoader
        val = COCOMaskLoader(anno_dir=args.anno_dir, img_dir=args.img_dir, split='val', data_type=args.data_type, category_filter=labels)
        data = TransformedDataset(val, coco_mask_example, n=args.eval_images or None)
    return InstanceSegmentationVOCEvaluator(data, faster_rcnn, label_names=labels)


def _all_rank_tickets(ticket, world, dev):
    """Every rank's loader ticket, in rank order (a collective when world > 1: called by all ranks)."""
    if world == 1:
        return [int(ticket)]
    t = torch.tensor([int(ticket)], dtype=torch.int64, device=dev if torch.distributed.get_backend() == 'nccl' else 'cpu')
    out = [torch.zeros_like(t) for _ in range(world)]
    torch.distributed.all_gather(out, t)
    return [int(o.item()) for o in out]


def _rank_ticket(saved, rank):
    """A trainer state holds one ticket per rank (older files: a single number = rank 0's)."""
    if isinstance(saved, (list, tuple)):
        return int(saved[rank]) if rank < len(saved) else int(saved[0])
    return int(saved)


class _Roctx(object):
    """roctx ranges through libroctx64 (ROCm's marker API; rocprofv3 --marker-trace shows them over the kernel trace)."""

    def __init__(self):
        import ctypes
        self.lib = None
        for name in ('librocprofiler-sdk-roctx.so', 'libroctx64.so'):
            try:
                self.lib = ctypes.CDLL(name)
                break
            except OSError:
                continue
        if self.lib is None:
            raise RuntimeError('--profile: neither librocprofiler-sdk-roctx.so nor libroctx64.so can be loaded')

    def range(self, name):
        rtx = self

        class _R(object):
            def __enter__(self_):
                rtx.lib.roctxRangePushA(name.encode())

            def __exit__(self_, *a):
                rtx.lib.roctxRangePop()
        return _R()


def main():
    args = build_parser().parse_args()
    print('lr:{}'.format(args.lr))
    print('output:{}'.format(args.out))
    print('iteration::{}'.format(args.iteration))
    print('backbone architecture:{}'.format(args.backbone))
    print('head architecture:{}'.format(args.head_arch))
    run(args)


if __name__ == '__main__':
    main()
