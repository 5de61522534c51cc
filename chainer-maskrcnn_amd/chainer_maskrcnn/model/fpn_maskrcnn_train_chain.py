"""The FPN Mask R-CNN training step on gfx950 kernels.

Mirror of chainer_maskrcnn/model/fpn_maskrcnn_train_chain.py:14-117: same constructor arguments,
``__call__(imgs, bboxes, labels, masks, scale) -> loss``, five un-weighted losses (:106), the same
report keys (:108-115; kept in ``self.observation`` as device scalars).  As in the reference the
``rpn_sigma`` / ``roi_sigma`` / ``anchor_target_creator`` arguments are accepted and the base-class
defaults (3, 1, default AnchorTargetCreator) apply (:19-26).

What is different in mechanism:
  * no host round trip: proposals, both target creators, the mask crop+resize and all losses run on
    the device; per-image counts stay on the device (padded rows carry label -1);
  * batch size > 1 (the reference raises for n != 1, :37-40; ``strict_batch1=True`` restores that):
    every image samples its own RoIs / anchors, the rows are concatenated and each loss is
    normalised over the concatenated batch (hard part 8);
  * the backward pass is an explicit tape walk (``backward()``); ``loss.backward()`` on the returned
    tensor triggers it, so reference-style ``loss = model(*batch); loss.backward()`` works;
  * the mask branch runs on the (<= 64 per image) positive rows only by default - identical loss and
    gradients; ``mask_rows='all'`` evaluates all sampled rows like the reference.
"""
import numpy as np
import torch

from chainer_maskrcnn._hip import ops
from chainer_maskrcnn.utils.proposal_target_creator import ProposalTargetCreator


class AnchorTargetCreator(object):
    """Parameters of ChainerCV's AnchorTargetCreator; the work is ops.anchor_target."""

    def __init__(self, n_sample=256, pos_iou_thresh=0.7, neg_iou_thresh=0.3, pos_ratio=0.5):
        self.n_sample, self.pos_iou_thresh, self.neg_iou_thresh, self.pos_ratio = n_sample, pos_iou_thresh, neg_iou_thresh, pos_ratio
        self.keys = ops.KeyStream(1 << 32)

    seed = property(lambda self: self.keys.seed)

    def set_seed(self, seed, device=None):
        self.keys.set_seed(seed, device)

    def __call__(self, bbox, anchor, img_size, n_gt=None, keys=None, per_image_hw=None):
        """bbox (N,G,4) (or (G,4)), anchor (A,4) -> (loc (N,A,4), label (N,A)).  per_image_hw (N,2): each image's own size."""
        if bbox.dim() == 2:
            bbox = bbox[None]
        N, G, _ = bbox.shape
        if n_gt is None:
            n_gt = torch.full((N,), G, dtype=torch.int32, device=bbox.device)
        if keys is None:
            keys = self.keys.draw((N, anchor.shape[0]), bbox.device)
        return ops.anchor_target(anchor, bbox.contiguous(), n_gt, img_size, keys, self.n_sample, self.pos_iou_thresh,
                                 self.neg_iou_thresh, self.pos_ratio, per_image_hw=per_image_hw)


class _LossHandle(torch.autograd.Function):
    """Makes ``loss.backward()`` on the returned scalar run the chain's explicit backward pass."""

    @staticmethod
    def forward(ctx, anchor, chain, value):
        ctx.chain = chain
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        # g = d(objective)/d(loss): 1 for a plain ``loss.backward()``; ``(loss * k).backward()`` (loss scaling) gives k.
        # MomentumSGD.update() calls loss.backward() itself and says so (unit_upstream), which skips the scaling pass.
        ctx.chain.backward(upstream=None if ctx.chain.unit_upstream else g)
        return None, None, None


def calc_mask_loss(roi_cls_mask, gt_roi_mask, xp, gt_roi_label):
    """train.py:50-58: channel ``gt_label - 1`` of every row, then sigmoid cross entropy of the first n_pos rows against
    the 28x28 targets.  Passed by name to FPNMaskRCNNTrainChain it is recognised (``fused_kind``) and evaluated as ONE
    fused kernel (``mrcnn_mask_bce_f32``: selection + loss + gradient); called directly - or copied into user code - the
    body below runs on the HIP-backed pieces of chainer_maskrcnn/functions/loss.py and gives the same value."""
    from chainer_maskrcnn import functions as F
    roi_mask = roi_cls_mask[xp.arange(roi_cls_mask.shape[0]), gt_roi_label - 1]
    return F.sigmoid_cross_entropy(roi_mask[:gt_roi_mask.shape[0]], gt_roi_mask)


calc_mask_loss.fused_kind = 'mask_bce'


def calc_keypoint_loss(roi_cls_mask, gt_roi_mask, xp, gt_roi_label, num_keypoints=17):
    """train_keypoints.py:21-27: softmax cross entropy over the 56*56 positions of each (positive RoI, keypoint).
    Fused form: ``mrcnn_softmax_ce_f32`` on the NHWC logits."""
    from chainer_maskrcnn import functions as F
    num_positives = gt_roi_mask.shape[0]
    roi_mask = roi_cls_mask[:num_positives].reshape((num_positives * num_keypoints, -1))
    return F.softmax_cross_entropy(roi_mask, gt_roi_mask.reshape((-1,)))


calc_keypoint_loss.fused_kind = 'keypoint_ce'


# Arithmetic of the convolution GEMMs (mrcnn_conv2d_set_split_operands: forward, backward-data, backward-filter; + which layers' FORWARD
# pass the setting applies to).  All of them take float32 tensors in and out and accumulate in float32:
#   'f32'                     v_mfma_f32_32x32x2_f32 in every pass (bit for bit an fmaf chain)
#   'bf16x6_behind_backbone'  the SHIPPED training default (train.py, bench.py): the float32-ACCURATE three-plane emulation on
#                             v_mfma_f32_32x32x16_bf16 - every operand carried exactly by three bf16 planes (hi + mid + lo), the six
#                             products of weight >= 2^-16 accumulated in float32; per-GEMM error against float64 <= the float32 MFMA's
#                             (tests/test_split_gemm_gpu.py) - in both backward passes of every layer and in the forward pass of every
#                             layer BEHIND the backbone (FPN, RPN, heads); the forward pass of the ResNet's convolutions stays on the
#                             float32 MFMA, so c2 .. c5 - 50 layers of training-mode BatchNorm - are those of the float32 step bit for
#                             bit.  Full-width parity with the UNRELAXED bars of the float32 configuration on five batches
#                             (tests/test_full_width_gpu.py; profiles/r04_full_width_parity_behind_backbone_forward_emulated.txt)
#   'bf16x6_backward'         float32 MFMA in the whole forward pass, the emulation in both backward passes (round 4's first choice: the
#                             same five batches pass, activations / losses / sampled targets bit-identical to 'f32')
#   'bf16x6'                  the emulation in every pass of every layer (opt-in: with the backbone's forward pass emulated, one of the
#                             five batches has 4 % of the gradient tensors above 3 x the float32 floor, against a 3 % bar)
# value = (split operands per pass, emulate the backbone's forward pass too)
GEMM_ARITHMETIC = {'f32': ((0, 0, 0), True), 'bf16x6_behind_backbone': ((3, 3, 3), False), 'bf16x6_backward': ((0, 3, 3), True),
                   'bf16x6': ((3, 3, 3), True)}
DEFAULT_GEMM_ARITHMETIC = 'bf16x6_behind_backbone'

# Box regression losses of the chain (box_loss, rpn_box_loss): the reference's smooth L1 on the encoded deltas, or an IoU loss on the decoded
# box (the kinds of ops.box_iou_loss)
BOX_LOSSES = ('smooth_l1', 'giou', 'diou', 'ciou')


def _weight(name, weight):
    """The one rule of the chain's loss weights: a finite number above 0, as a float."""
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not np.isfinite(weight) or weight <= 0:
        raise ValueError('%s must be a finite number above 0, got %r' % (name, weight))
    return float(weight)


def box_loss_settings(box_loss='smooth_l1', rpn_box_loss='smooth_l1', box_loss_weight=1.0, rpn_box_loss_weight=1.0):
    """The four box-loss arguments of FPNMaskRCNNTrainChain as a dict, checked (the constructor and train.py's flags share the rule):
    ValueError for a name outside BOX_LOSSES, a weight that is not a finite number above 0, a weight other than 1.0 with 'smooth_l1'."""
    for arg, name, weight in (('box_loss', box_loss, box_loss_weight), ('rpn_box_loss', rpn_box_loss, rpn_box_loss_weight)):
        if name not in BOX_LOSSES:
            raise ValueError('%s must be one of %s, got %r' % (arg, list(BOX_LOSSES), name))
        _weight(arg + '_weight', weight)
        if name == 'smooth_l1' and weight != 1.0:
            raise ValueError("%s_weight applies to giou / diou / ciou; %s='smooth_l1' takes 1.0 only, got %r" % (arg, arg, weight))
    return dict(box_loss=box_loss, rpn_box_loss=rpn_box_loss, box_loss_weight=float(box_loss_weight),
                rpn_box_loss_weight=float(rpn_box_loss_weight))


def mask_iou_weight_setting(weight):
    """The mask_iou_weight argument of FPNMaskRCNNTrainChain as a float, checked like the box-loss weights: ValueError unless it is a finite
    number above 0."""
    return _weight('mask_iou_weight', weight)


def point_loss_weight_setting(weight):
    """The point_loss_weight argument of FPNMaskRCNNTrainChain as a float, checked like mask_iou_weight: ValueError unless it is a finite
    number above 0."""
    return _weight('point_loss_weight', weight)


def loss_rows(later_stages, mask_iou=False, point=False):
    """The rows of the step's ``losses`` tensor: ([(observation key, row), ...] in row order, number of rows).  The reference's five, then a
    (loc, cls) pair per box stage behind the first (Cascade R-CNN: stages 2 .. 1 + later_stages), the MaskIoU head's, the point head's."""
    rows = [('rpn_loc_loss', 0), ('rpn_cls_loss', 1), ('roi_loc_loss', 2), ('roi_cls_loss', 3), ('mask_loss', 4)]
    for k in range(2, 2 + later_stages):
        loc = 5 + 2 * (k - 2)
        rows += [('roi_loc_loss_s%d' % k, loc), ('roi_cls_loss_s%d' % k, loc + 1)]
    for key, present in (('maskiou_loss', mask_iou), ('point_loss', point)):
        if present:
            rows.append((key, len(rows)))
    return rows, len(rows)


def select_gemm_arithmetic(name):
    """Process-wide: the library's split-operand modes and the per-layer rule of nn/core.py."""
    from chainer_maskrcnn._hip import lib, check
    from chainer_maskrcnn.nn import core
    split, backbone_fwd = GEMM_ARITHMETIC[name]
    check(lib().mrcnn_conv2d_set_split_operands(*split))
    core.FWD_EMULATION_IN_BACKBONE = bool(backbone_fwd)


class _PendingBackward(object):
    """What a forward pass leaves for backward(): the pyramid and the loss gradients the tape walk starts from."""

    def __init__(self, features, g_locs, g_scores, g_box, g_mask, g_later, g_iou, point, early_rpn):
        self.features = features
        self.g_locs, self.g_scores = g_locs, g_scores       # RPN: (n, A, 4) and (n, A, 2)
        self.g_box, self.g_mask = g_box, g_mask             # the head's box and mask outputs
        self.g_later = g_later          # the later box stages' loss gradients, in stage order
        self.g_iou = g_iou              # the MaskIoU loss gradient (None without the head)
        self.point = point              # the point head's coords, rois and loss gradient 'g_pred' (None without the head)
        self.early_rpn = early_rpn      # the RPN's per-level feature gradients where its backward pass ran in the forward pass, or None

    def seeds(self):
        """Every loss gradient, for the upstream-scaling pass."""
        return ([self.g_locs, self.g_scores, self.g_box, self.g_mask] + list(self.g_later) + ([self.g_iou] if self.g_iou is not None else [])
                + ([self.point['g_pred']] if self.point is not None else []))


class FPNMaskRCNNTrainChain(object):
    EARLY_RPN_BACKWARD = True      # A/B switch of the early RPN backward (see _rpn_loss_branch)
    # (r6) the heads' ROIAlign backward passes ACCUMULATE into the feature gradients the early RPN backward left (the kernel then touches
    # only the patches RoIs land on instead of writing every map), instead of five add_ kernels over the pyramid afterwards: same sums in
    # another order - (rpn + box) + mask instead of (box + mask) + rpn -, 0.5 GB and 5 launches less on the main stream
    ACCUMULATE_INTO_EARLY_RPN = True

    def __init__(self, faster_rcnn, mask_loss_fun=calc_mask_loss, binary_mask=True, rpn_sigma=3., roi_sigma=1.,
                 anchor_target_creator=None, strict_batch1=False, mask_rows='positives', gemm_arithmetic=None,
                 box_loss='smooth_l1', rpn_box_loss='smooth_l1', box_loss_weight=1.0, rpn_box_loss_weight=1.0, mask_iou_weight=1.0,
                 point_loss_weight=1.0):
        """gemm_arithmetic: a key of GEMM_ARITHMETIC - the chain then selects it (process-wide library setting) at the start of every
        step; None (default of this constructor, used by the kernel-level tests) leaves the process setting alone.  train.py and
        bench.py pass DEFAULT_GEMM_ARITHMETIC.

        box_loss / rpn_box_loss: the box regression loss of the RoI head / the RPN, one of BOX_LOSSES.  'smooth_l1' (default) is the
        reference's loss on the encoded deltas; 'giou', 'diou', 'ciou' decode prediction and target against the sampled RoI / the anchor
        and take the loss on the boxes (ops.box_iou_loss) - same targets, same normaliser, same report keys.
        box_loss_weight / rpn_box_loss_weight multiply that loss and its gradient; smooth L1 takes no weight (1.0 only).

        mask_iou_weight: multiplies the MaskIoU head's L2 loss and its gradient (a finite number above 0; Mask Scoring R-CNN, DESIGN.md
        section 3.22).  It acts on a model built with ``mask_iou=True`` only: the chain then runs target -> input assembly -> head -> L2
        behind the mask loss and reports ``maskiou_loss``.

        point_loss_weight: multiplies the point head's loss and its gradient (a finite number above 0; PointRend).
        It acts on a model built with ``point_rend=True`` only: the chain then runs points -> features -> head -> target -> loss behind the
        mask loss, on the mask branch's rows, and reports ``point_loss``."""
        box_loss_settings(box_loss, rpn_box_loss, box_loss_weight, rpn_box_loss_weight)
        self.mask_iou_weight = mask_iou_weight_setting(mask_iou_weight)
        self.point_loss_weight = point_loss_weight_setting(point_loss_weight)
        self.box_loss, self.rpn_box_loss = box_loss, rpn_box_loss
        self.box_loss_weight, self.rpn_box_loss_weight = float(box_loss_weight), float(rpn_box_loss_weight)
        if gemm_arithmetic is not None and gemm_arithmetic not in GEMM_ARITHMETIC:
            raise ValueError('gemm_arithmetic must be one of %s' % sorted(GEMM_ARITHMETIC))
        self.gemm_arithmetic = gemm_arithmetic
        self.faster_rcnn = faster_rcnn
        self.proposal_target_creator = ProposalTargetCreator(faster_rcnn.extractor.anchor_sizes)
        self.anchor_target_creator = AnchorTargetCreator()      # the argument is ignored, as in the reference
        cascade = getattr(faster_rcnn, 'cascade', None)
        if cascade is not None and cascade[0][0] != float(self.proposal_target_creator.pos_iou_thresh):
            raise ValueError('cascade_ious[0] = %r is not the sampler\'s pos_iou_thresh %r'
                             % (cascade[0][0], self.proposal_target_creator.pos_iou_thresh))
        self.rpn_sigma, self.roi_sigma = 3., 1.                  # base-class defaults apply (:25-26)
        self.loc_normalize_mean = faster_rcnn.loc_normalize_mean
        self.loc_normalize_std = faster_rcnn.loc_normalize_std
        if not callable(mask_loss_fun):
            raise TypeError('mask_loss_fun must be callable: f(roi_cls_mask, gt_roi_mask, xp, gt_roi_label) -> loss')
        # the two functions of the reference's train scripts are recognised and run as fused kernels; any other callable
        # is CALLED, like the reference does (:103-104), on device tensors (see _generic_mask_loss)
        self.mask_loss_fun = mask_loss_fun
        self.mask_loss_kind = getattr(mask_loss_fun, 'fused_kind', None)
        if self.mask_loss_kind not in ('mask_bce', 'keypoint_ce'):
            self.mask_loss_kind = 'generic'
        if getattr(faster_rcnn, 'maskiou_head', None) is not None and self.mask_loss_kind != 'mask_bce':
            raise ValueError('a mask_iou model trains with the fused binary mask loss (calc_mask_loss): a user-supplied mask_loss_fun '
                             're-orders the mask rows, which the MaskIoU target does not follow')
        if getattr(faster_rcnn, 'point_head', None) is not None and self.mask_loss_kind != 'mask_bce':
            raise ValueError('a point_rend model trains with the fused binary mask loss (calc_mask_loss): a user-supplied mask_loss_fun '
                             're-orders the mask rows, which the point targets do not follow')
        self.unit_upstream = False
        self.backward_follows = False       # set by MomentumSGD.update around its forward call: loss.backward() comes next, with d loss = 1
        self.binary_mask = binary_mask
        self.strict_batch1 = strict_batch1
        self.mask_rows = mask_rows
        self.observation = {}
        self.grad_ready_hook = None         # called with the lowest finished parameter offset during backward (DP overlap)
        self.sampler_keys = None            # (proposal keys, anchor keys) override for parity tests
        self.point_keys = None              # (mask rows, ops.point_n_keys) int32 keys of the PointRend training points, for parity tests
        self._point_stream = ops.KeyStream(1 << 33)     # the point keys are drawn from it
        self.use_aux_stream = True          # independent branches (RPN losses, box head) on a second compute stream
        self.keep_outputs = False           # parity tests: keep the head outputs of the last step in self.outputs
        self.outputs = {}
        self._aux = {}
        # Cascade R-CNN: the box stages behind the head; Mask Scoring R-CNN: the MaskIoU head (section 3.22);
        # PointRend: the point head (section 3.24).  Their loss rows follow the reference's five, in this order
        self._loss_rows, self._n_loss_rows = loss_rows(len(getattr(faster_rcnn, 'cascade_heads', [])),
                                                       getattr(faster_rcnn, 'maskiou_head', None) is not None,
                                                       getattr(faster_rcnn, 'point_head', None) is not None)
        self._row = dict(self._loss_rows)
        self.pending = None                 # the _PendingBackward of a forward pass whose backward pass has not run yet
        self._mask_active = None            # active-row mask of the pending mask branch backward (_mask_loss; None = dense)
        self._arith_found = None            # the process's GEMM arithmetic before this chain selected its own (restored by backward())

    @property
    def key_streams(self):
        """The chain's ops.KeyStream objects by their names in the trainer state (MomentumSGD.state_dict, 'samplers')."""
        streams = {'proposal_target_creator': self.proposal_target_creator.keys, 'anchor_target_creator': self.anchor_target_creator.keys}
        if getattr(self.faster_rcnn, 'point_head', None) is not None:
            streams['point_rend'] = self._point_stream
        return streams

    def _aux_stream(self, dev):
        key = (dev.type, dev.index)
        if key not in self._aux:
            self._aux[key] = torch.cuda.Stream(device=dev)
        return self._aux[key]

    # ------------------------------------------------------------------------------------------
    def __call__(self, imgs, bboxes, labels, masks, scale, n_gt=None, img_sizes=None):
        """scale: the Transform's resize factor - a number, or one per image (host array or device tensor).  img_sizes:
        optional (N,2) (h, w) of every image inside the zero-padded batch tensor (dataset/loader.py 'sizes'); with either,
        proposals are clipped to / anchors tested against each image's OWN size and min_size * its own scale, which is
        what the reference's batch-1-per-process step does (fpn_maskrcnn_train_chain.py:60-70)."""
        m = self.faster_rcnn
        n = bboxes.shape[0]
        if self.strict_batch1 and n != 1:
            raise ValueError('Currently only batch size 1 is supported. n={}'.format(n))
        if self.gemm_arithmetic is not None:        # (read by the library on the host at call time: forward now, backward later)
            # the process-wide setting this chain found is put back at the end of backward(): evaluation / predict calls between training
            # steps and other models of the process keep THEIR arithmetic
            if self._arith_found is None:
                from chainer_maskrcnn._hip import nn as hnn
                from chainer_maskrcnn.nn import core
                self._arith_found = (hnn.split_operands(), core.FWD_EMULATION_IN_BACKBONE)
            select_gemm_arithmetic(self.gemm_arithmetic)
        if torch.is_tensor(scale) and scale.numel() == 1:
            scale = float(scale.reshape(-1)[0].item())
        dev = imgs.device
        _, _, H, W = imgs.shape
        img_size = (H, W)
        per_hw = None
        if img_sizes is not None:
            per_hw = (img_sizes if torch.is_tensor(img_sizes) else torch.from_numpy(np.asarray(img_sizes, np.float32))).to(dev, torch.float32).contiguous()
        i32 = torch.int32
        bboxes = bboxes.contiguous()
        labels = labels.to(i32).contiguous()
        if n_gt is None:
            # padded batches (Chainer's concat_examples / dataset/loader.py pad ragged images with label -1 and zero
            # boxes): the valid rows are packed first, so the per-image count is #(label >= 0) - counted on the device
            n_gt = ops.count_valid_labels(labels)

        main = torch.cuda.current_stream(dev)
        aux = self._aux_stream(dev) if self.use_aux_stream else main
        if getattr(m.head, 'merge_deconv', False):      # composed deconv1*conv2 weights: ready long before the mask branch
            aux.wait_stream(main)
            with torch.cuda.stream(aux):
                m.head.compose_deconv(dev)
        features = m.extractor(m.to_nhwc4(imgs))
        m.rpn.train = True
        pk, ak = self.sampler_keys if self.sampler_keys is not None else (None, None)
        losses = torch.empty((self._n_loss_rows, 2), dtype=torch.float32, device=dev)
        rpn = {}

        def rpn_loss_branch(locs, scores, anchors):
            rpn.update(self._rpn_loss_branch(locs, scores, anchors, bboxes, img_size, n_gt, ak, per_hw, losses, main, aux))

        r = m.rpn.forward_padded(features, per_hw if per_hw is not None else img_size, scale, after_heads=rpn_loss_branch, batch_size=img_size)
        A = r['anchors'].shape[0]
        # Branch 2 (main stream): proposals -> sampled RoIs and targets
        t = self.proposal_target_creator.sample_batch(
            r['rois'], r['levels'], r['n_rois'], bboxes, labels, n_gt,
            masks=masks.contiguous() if self.binary_mask else None,
            keypoints=None if self.binary_mask else masks.contiguous(),
            loc_normalize_mean=self.loc_normalize_mean, loc_normalize_std=self.loc_normalize_std,
            mask_size=m.head.mask_size, keys=pk, mask_rows=self.mask_rows)

        # head (:88-89) on the n*n_sample sampled rows (padding rows have label -1 and get zero gradient): the box branch
        # runs on the aux stream concurrently with the (much larger) mask branch on the main stream
        scales = m.extractor.spatial_scales
        aux.wait_stream(main)
        with torch.cuda.stream(aux):
            box, g_boxes, casc = self._box_stages(features, t, scales, bboxes, labels, n_gt,
                                                  per_hw if per_hw is not None else (float(H), float(W)), losses)
        m_rois, m_levels, m_label, mask_out, g_mask = self._mask_loss(features, t, scales, losses)
        iou = self._maskiou_branch(masks, n_gt, t, m_label, mask_out, losses) if getattr(m, 'maskiou_head', None) is not None else None
        pt = (self._point_branch(masks, n_gt, t, m_rois, m_label, mask_out, features, scales, losses)
              if getattr(m, 'point_head', None) is not None else None)

        main.wait_stream(aux)
        if aux is not main:             # allocated on the aux stream, consumed by the RPN backward on the main stream
            rpn['g_locs'].record_stream(main)
            rpn['g_scores'].record_stream(main)
        total = ops.loss_total(losses)
        self.pending = _PendingBackward(features, rpn['g_locs'].view(n, A, 4), rpn['g_scores'].view(n, A, 2), g_boxes[0], g_mask, g_boxes[1:],
                                        iou['g_pred'] if iou is not None else None, pt, rpn.get('g_feats'))
        self._publish(losses, total, features, r, box, mask_out, casc, g_boxes, iou, pt, g_mask)
        self.targets = t
        self.rpn_targets = (rpn['loc'], rpn['label'])
        self.mask_inputs = (m_rois, m_levels, m_label)
        self.rpn_out = r
        self._anchor = torch.zeros((), device=dev, requires_grad=True)
        return _LossHandle.apply(self._anchor, self, total[0])

    def backward(self, upstream=None):
        """Explicit backward pass: fills the flat gradient buffer of ``faster_rcnn.ps``.  ``upstream`` (device scalar or
        None = 1): d(objective)/d(loss), multiplied into the loss-gradient seeds."""
        m = self.faster_rcnn
        st = self.pending
        features = st.features
        if upstream is not None:
            from chainer_maskrcnn.functions.loss import _scale_
            for g_ in st.seeds():
                _scale_(g_, upstream)
        hook = self.grad_ready_hook
        dev = features[0].device
        main = torch.cuda.current_stream(dev)
        aux = self._aux_stream(dev) if self.use_aux_stream else main
        into_early = (self.ACCUMULATE_INTO_EARLY_RPN and st.early_rpn is not None and upstream is None
                      and len(st.early_rpn) == len(features))
        if into_early:
            g_feats = list(st.early_rpn)
            for g in g_feats:
                g.record_stream(main)
        else:
            g_feats = [torch.empty_like(f) for f in features]
        aux.wait_stream(main)
        with torch.cuda.stream(aux):
            self._box_stages_backward(st, g_feats, into_early)
        # the MaskIoU head first (main stream): its parameter gradients are final and its input gradient is at hand before the mask
        # branch's; the feature part joins the mask convolutions' pooled gradient, so the ONE ROIAlign backward below carries both
        g_iou_in = m.maskiou_head.backward(st.g_iou) if st.g_iou is not None else None
        # the point head likewise (main stream): its input gradient waits for the ROIAlign backward passes below
        g_pt_in = m.point_head.backward(st.point['g_pred']) if st.point is not None else None
        active = self._mask_active
        self._mask_active = None
        g_pool = m.head.backward_mask_convs(st.g_mask, active=active)    # main stream: the mask branch down to its pooled input
        if g_iou_in is not None:
            self._maskiou_input_backward(g_iou_in, g_pool)
        main.wait_stream(aux)
        if self.keep_outputs and g_iou_in is not None:       # parity tests: the pyramid gradient the box stages left
            self.outputs.update(g_feats_box=[g.clone() for g in g_feats])
        m.head.backward_mask_pool(g_pool, g_feats, active=active)        # accumulates into g_feats (second pooled size)
        if g_pt_in is not None:
            self._point_input_backward(st.point, g_pt_in, g_feats)
        if self.keep_outputs and (st.g_later or g_iou_in is not None):       # parity tests: the mask branch's pooled gradient and the pyramid gradient behind the heads
            self.outputs.update(g_mask_pool=g_pool, g_feats_heads=[g.clone() for g in g_feats])
        if hook:
            hook(self._offset_of('head/'))
        self._rpn_backward(st, g_feats, into_early, upstream, main)
        if hook:
            hook(self._offset_of('rpn/'))
        m.extractor.backward(g_feats, progress=(lambda prefix: hook(self._offset_of(prefix))) if hook else None)
        from chainer_maskrcnn.nn import core
        core.join_side_stream(features[0].device)
        if hook:
            hook(0)
        self.pending = None
        if self._arith_found is not None:
            from chainer_maskrcnn._hip import lib, check
            split, in_backbone = self._arith_found
            check(lib().mrcnn_conv2d_set_split_operands(*split))
            core.FWD_EMULATION_IN_BACKBONE = in_backbone
            self._arith_found = None

    # ---- the stages of the step: each forward piece, then its backward piece ---------------------------------------------
    def _rpn_loss_branch(self, locs, scores, anchors, bboxes, img_size, n_gt, keys, per_hw, losses, main, aux):
        """Branch 1 (aux stream): anchor targets + RPN losses (:81-85).  It needs the RPN head outputs only, so it is
        enqueued before the proposal kernels and runs beside them.  -> loc, label, g_locs, g_scores (and g_feats, below)."""
        m, row, br1 = self.faster_rcnn, self._row, {}
        n, A_ = bboxes.shape[0], anchors.shape[0]
        aux.wait_stream(main)
        with torch.cuda.stream(aux):
            br1['loc'], br1['label'] = self.anchor_target_creator(bboxes, anchors, img_size, n_gt=n_gt, keys=keys, per_image_hw=per_hw)
            if self.rpn_box_loss == 'smooth_l1':
                _, br1['g_locs'] = ops.smooth_l1(locs.view(n * A_, 4), 4, br1['loc'].view(n * A_, 4), br1['label'].view(-1),
                                                 n * A_, self.rpn_sigma, out=losses[row['rpn_loc_loss']])
            else:   # on the decoded box: every image's rows are relative to the shared anchors; the RPN's targets are not normalised
                _, br1['g_locs'] = ops.box_iou_loss(locs.view(n * A_, 4), 4, br1['loc'].view(n * A_, 4), anchors, br1['label'].view(-1),
                                                    n * A_, self.rpn_box_loss, (0., 0., 0., 0.), (1., 1., 1., 1.),
                                                    weight=self.rpn_box_loss_weight, roi_period=A_, out=losses[row['rpn_loc_loss']])
            _, br1['g_scores'] = ops.softmax_ce(scores.view(n * A_, 2), br1['label'].view(-1), n * A_, 2, (1, 2, 0, 1),
                                                out=losses[row['rpn_cls_loss']])
            # The RPN's own backward pass needs nothing but these two gradients: when a backward pass is known to follow
            # (MomentumSGD.update) it is enqueued HERE, on the aux stream, and fills the chip while the main stream walks the
            # latency-bound proposal chain (decode, select, sort, NMS, target sampling: small kernels on a few CUs).  Its
            # per-level feature gradients are kept and added in backward() where rpn.backward() used to run.
            if self.EARLY_RPN_BACKWARD and self.backward_follows and aux is not main:
                for c1, c2, _, _ in m.rpn.tape:         # saved activations were allocated on the main stream and are released by
                    for t_ in tuple(c1) + tuple(c2):    # this call: the allocator must not hand them out again before aux is done
                        if torch.is_tensor(t_):
                            t_.record_stream(aux)
                br1['g_feats'] = m.rpn.backward(br1['g_locs'].view(n, A_, 4), br1['g_scores'].view(n, A_, 2), None)
        return br1

    def _rpn_backward(self, st, g_feats, into_early, upstream, main):
        """The RPN's part of g_feats, behind the heads': already in them (into_early), added from the early pass, or computed now."""
        if into_early:
            st.early_rpn = None
        elif st.early_rpn is not None:        # computed beside the proposal chain of the forward pass (aux stream, joined at its end)
            if upstream is not None:        # (its parameter gradients are already in the buffer, un-scaled: they cannot be fixed up here)
                raise RuntimeError('the RPN backward pass ran early with d(objective)/d(loss) = 1 (backward_follows was set): '
                                   'a scaled loss needs chain.backward_follows = False during the forward call')
            for gf, g in zip(g_feats, st.early_rpn):
                gf.add_(g)
                g.record_stream(main)
            st.early_rpn = None
        else:
            self.faster_rcnn.rpn.backward(st.g_locs, st.g_scores, g_feats)

    def _box_stage_losses(self, box, roi, gt_loc, label, std, loc_row, cls_row):
        """The two losses of one box stage on its output ``box`` (R, head.out_p) -> their gradient: softmax cross entropy over the class
        columns, then smooth L1 on the encoded deltas or - an IoU loss - on the decoded box, against ``roi``, the box the stage's targets
        ``gt_loc`` were encoded with, and the stage's ``std``.  Every stage normalises by the same (sum, count)."""
        head = self.faster_rcnn.head
        R, ld = label.shape[0], head.out_p
        g_box = torch.empty_like(box)
        ops.softmax_ce(box, label, R, head.n_class, (1, ld, 0, 1), Kfill=head.LOC0, gx=g_box, out=cls_row)
        if self.box_loss == 'smooth_l1':
            ops.smooth_l1(box, ld, gt_loc, label, R, self.roi_sigma, gfill=ld - head.LOC0, col0=head.LOC0, gx=g_box, out=loc_row)
        else:
            ops.box_iou_loss(box, ld, gt_loc, roi, label, R, self.box_loss, self.loc_normalize_mean, std, weight=self.box_loss_weight,
                             roi_period=R, gfill=ld - head.LOC0, col0=head.LOC0, gx=g_box, out=loc_row)
        return g_box

    def _box_stages(self, features, t, scales, bboxes, labels, n_gt, img_hw, losses):
        """The head's box branch and, behind it on the same stream, the cascade's -> (stage 1's output, every stage's loss gradient,
        the later stages' refine outputs + 'box')."""
        m, row = self.faster_rcnn, self._row
        head, n = m.head, bboxes.shape[0]
        box = head.box_branch(features, t['rois_xy5'], t['sample_levels'], scales)
        g_boxes = [self._box_stage_losses(box, t['sample_roi'], t['gt_roi_loc'], t['gt_roi_label'], self.loc_normalize_std,
                                          losses[row['roi_loc_loss']], losses[row['roi_cls_loss']])]
        # Stage k >= 2, behind stage k-1 on the same stream and the same N * n_sample rows (no resampling, no host sync): stage k-1's
        # input boxes refined by its own deltas, re-levelled, re-matched at the stage's IoU threshold and re-encoded with the stage's
        # std - a constant: no gradient flows through the refinement -, then the stage's box branch and the two losses of stage 1
        casc = []
        prev = dict(roi=t['sample_roi'], label=t['gt_roi_label'], box=box)
        for k, stage in enumerate(getattr(m, 'cascade_heads', []), 2):
            ious, stds = m.cascade
            ref = ops.cascade_refine(prev['roi'], prev['box'], head.LOC0, n, self.loc_normalize_mean, stds[k - 2], img_hw,
                                     prev_label=prev['label'], gt_boxes=bboxes, gt_labels=labels, n_gt=n_gt, iou_thresh=ious[k - 1],
                                     std_next=stds[k - 1])
            ref['box'] = stage.box_branch(features, ref['rois_xy5'], ref['levels'], scales)
            g_boxes.append(self._box_stage_losses(ref['box'], ref['roi'], ref['gt_loc'], ref['label'], stds[k - 1],
                                                  losses[row['roi_loc_loss_s%d' % k]], losses[row['roi_cls_loss_s%d' % k]]))
            casc.append(ref)
            prev = ref
        return box, g_boxes, casc

    def _box_stages_backward(self, st, g_feats, into_early):
        m = self.faster_rcnn
        m.head.backward_box(st.g_box, g_feats, accumulate=into_early)     # overwrites g_feats (first pooled size) unless they hold the RPN's
        for stage, g_k in zip(getattr(m, 'cascade_heads', []), st.g_later):      # the later box stages add theirs, in stage order
            stage.backward_box(g_k, g_feats, accumulate=True)

    def _mask_loss(self, features, t, scales, losses):
        """The mask branch on its rows and the mask loss -> (the rows' rois, levels and labels, the NHWC logits, the loss gradient)."""
        from chainer_maskrcnn.nn import core
        from chainer_maskrcnn._hip import nn as hnn
        head = self.faster_rcnn.head
        self._mask_active = None
        if self.mask_loss_kind == 'generic':
            g_mask = self._generic_mask_loss(t, features, scales, losses)
            return self._generic_inputs + (None, g_mask)
        S, rows = self.proposal_target_creator.n_sample, t['mask_rows']
        n = t['rois_xy5'].shape[0] // S
        if rows == S:
            m_rois, m_levels, m_label = t['rois_xy5'], t['sample_levels'], t['gt_roi_label']
        else:   # the first `rows` rows of every image block (positives come first)
            m_rois = t['rois_xy5'].view(n, S, 5)[:, :rows].reshape(n * rows, 5)
            m_levels = t['sample_levels'].view(n, S)[:, :rows].reshape(n * rows)
            m_label = t['gt_roi_label'].view(n, S)[:, :rows].reshape(n * rows)
        mask_out = head.mask_branch(features, m_rois, m_levels, scales)
        out = losses[self._row['mask_loss']]
        if self.mask_loss_kind == 'mask_bce':
            _, g_mask = ops.mask_bce(mask_out, t['gt_roi_mask'], m_label, out=out)
            # mask_rows='all': the loss reads the first n_pos rows of every image block only (label <= 0 behind them), so g_mask is an exact
            # zero on the others and the backward pass may leave them out.  Not with a MaskIoU or PointRend head: their gradients reach
            # the mask branch on rows of their own choosing.  The mask is built on this stream, beside the loss; n_pos stays on the device.
            m = self.faster_rcnn
            if (rows == S and core.MASK_BWD_SKIP_INACTIVE and getattr(m, 'maskiou_head', None) is None
                    and getattr(m, 'point_head', None) is None):
                self._mask_active = hnn.active_rows(t['n_pos'].to(torch.int32).contiguous(), S)
        else:
            Rm, Hm, Wm, Cm = mask_out.shape
            K = head.n_keypoints
            xmap = (K, Hm * Wm * Cm, 1, Cm)
            g_mask = torch.empty_like(mask_out) if ops.softmax_ce_fills_gradient(Rm * K, Hm * Wm, xmap) else torch.zeros_like(mask_out)
            ops.softmax_ce(mask_out, t['gt_roi_mask'].view(-1), Rm * K, Hm * Wm, xmap, gx=g_mask, out=out)
        return m_rois, m_levels, m_label, mask_out, g_mask

    def _generic_mask_loss(self, t, features, scales, losses):
        """A user-supplied ``mask_loss_fun`` (not one of the two recognised functions): call it like the reference does
        (:103-104) - ``roi_cls_mask`` (R, C, S, S) with the positive rows first, ``gt_roi_mask`` with exactly n_pos rows,
        ``xp``, ``gt_roi_label`` (R,) - under torch autograd on HIP-backed operators (functions/loss.py), and return the
        gradient w.r.t. the NHWC logits.  Exact row counts need one host sync; this is the compatibility path."""
        from chainer_maskrcnn.functions import loss as FL
        m = self.faster_rcnn
        head = m.head
        S = self.proposal_target_creator.n_sample
        n = t['n_pos'].shape[0]
        n_pos = [int(v) for v in t['n_pos'].cpu().tolist()]
        n_smp = [int(v) for v in t['n_sampled'].cpu().tolist()]
        rows_of = lambda x, lo, hi: [x.view(n, S, *x.shape[1:])[i, lo(i):hi(i)] for i in range(n)]
        order = lambda x: torch.cat(rows_of(x, lambda i: 0, lambda i: n_pos[i]) +
                                    rows_of(x, lambda i: n_pos[i], lambda i: n_smp[i]), 0).contiguous()
        m_rois, m_levels, m_label = order(t['rois_xy5']), order(t['sample_levels']), order(t['gt_roi_label'])
        rows = t['mask_rows']
        gt = t['gt_roi_mask']
        gt = torch.cat([gt.view(n, rows, *gt.shape[1:])[i, :n_pos[i]] for i in range(n)], 0).contiguous()
        self._generic_inputs = (m_rois, m_levels, m_label)
        mask_out = head.mask_branch(features, m_rois, m_levels, scales)          # (R, S, S, Cp) NHWC
        leaf = mask_out.detach().requires_grad_(True)
        C = head.mask_out_channels
        with torch.enable_grad():
            x = FL.nhwc_to_nchw(leaf, C).as_subclass(FL.MaskLogits)
            loss = self.mask_loss_fun(x, gt, FL.XP(leaf.device), m_label)
            if not torch.is_tensor(loss) or loss.numel() != 1:
                raise TypeError('mask_loss_fun must return a scalar tensor')
            (g_mask,) = torch.autograd.grad(loss.reshape(()), leaf)
        out = losses[self._row['mask_loss']]
        out[0].copy_(loss.detach().reshape(()))
        out[1].fill_(1.0)
        return g_mask.contiguous()

    def _maskiou_branch(self, masks, n_gt, t, m_label, mask_out, losses):
        """Behind the mask loss, on the main stream and the mask branch's own rows: the IoU of each row's thresholded logits with its
        ground truth (integer counts), the head's input (pooled features + the max-pooled class logit, a constant), the head, the L2
        loss over the rows that have a target.  No host synchronisation.  -> target, area, (counts,) input, pred, g_pred."""
        m = self.faster_rcnn
        mh, S = m.maskiou_head, self.proposal_target_creator.n_sample
        m_label = m_label.contiguous()
        iou = ops.maskiou_target(masks.contiguous(), n_gt, t['sample_roi'], t['gt_assign'], m_label, t['n_pos'], S, t['mask_rows'], mask_out,
                                 t['gt_roi_mask'], mh.out_channels, label_base=1, want_counts=self.keep_outputs)
        iou['input'] = mh.assemble(m.head.last_mask_pool, mask_out, m_label, label_base=1)
        iou['pred'] = mh.forward(iou['input'])
        _, iou['g_pred'] = ops.maskiou_l2(iou['pred'], iou['target'], m_label, mh.out_channels, weight=self.mask_iou_weight, label_base=1,
                                          out=losses[self._row['maskiou_loss']])
        return iou

    def _maskiou_input_backward(self, g_iou_in, g_pool):
        if self.keep_outputs:       # parity tests: the two summands
            self.outputs.update(g_mask_pool_convs=g_pool.clone(), g_maskiou_in=g_iou_in)
        ops.maskiou_input_bwd(g_iou_in, g_pool)

    def _point_branch(self, masks, n_gt, t, m_rois, m_label, mask_out, features, scales, losses):
        """Behind the mask loss, on the main stream and the mask branch's own rows: the training points from the coarse logits'
        uncertainty, the head's input sampled from the stride-4 level and the logits (constants for the head), the head, the soft
        targets from the ground-truth masks, the loss over the live rows.  No host synchronisation.  -> coords, rois, input, pred,
        target, g_pred."""
        m = self.faster_rcnn
        ph, st, S = m.point_head, m.point_rend, self.proposal_target_creator.n_sample
        m_label, m_rois = m_label.contiguous(), m_rois.contiguous()
        keys = self.point_keys
        if keys is None:
            keys = self._point_stream.draw((mask_out.shape[0], ops.point_n_keys(st['train_points'], st['n_candidates'], st['n_important'])),
                                           mask_out.device)
        pt = dict(coords=ops.point_train_coords(keys, mask_out, m_label, ph.out_channels, st['train_points'], st['n_candidates'],
                                                st['n_important'], label_base=1), rois=m_rois)
        pt['input'] = ph.assemble(pt['coords'], m_rois, features[0], scales[0], mask_out)
        pt['pred'] = ph.forward(pt['input'])
        pt['target'] = ops.point_target(masks.contiguous(), n_gt, m_rois, t['gt_assign'], m_label, t['n_pos'], S, t['mask_rows'], pt['coords'])
        _, pt['g_pred'] = ops.point_bce(pt['pred'], pt['target'], m_label, ph.out_channels, weight=self.point_loss_weight, label_base=1,
                                        out=losses[self._row['point_loss']])
        return pt

    def _point_input_backward(self, pt, g_pt_in, g_feats):
        """PointRend: the fine part of the point head's input gradient, added into the stride-4 level's gradient behind the heads' ROIAlign
        backward passes (and the RPN's, where it ran early) - what the map holds is the first addend, then ascending (row, point)."""
        if self.keep_outputs:       # parity tests: the map before the addition and the addend
            pt['g_in'] = g_pt_in
            self.outputs.update(g_feats0_heads=g_feats[0].clone())
        ops.point_features_bwd(g_pt_in, pt['coords'], pt['rois'], self.faster_rcnn.extractor.spatial_scales[0], g_feats[0])
        if self.keep_outputs:
            self.outputs.update(g_feats0_point=g_feats[0].clone())

    def _publish(self, losses, total, features, r, box, mask_out, casc, g_boxes, iou, pt, g_mask):
        """``observation`` (device scalars; 'loss' sixth, behind the reference's five) and, for the parity tests, ``outputs``."""
        self.observation = {}
        for key, row in self._loss_rows:
            self.observation[key] = losses[row, 0]
            if key == 'mask_loss':
                self.observation['loss'] = total[0]
        if self.keep_outputs:
            self.outputs = dict(features=features, locs=r['locs'], scores=r['scores'], box=box, mask=mask_out)
            if casc:        # per later stage: the refine outputs (roi, rois_xy5, levels, gt_loc, label, gt_assign) and 'box'; every stage's loss gradient
                self.outputs.update(cascade=casc, g_boxes=g_boxes, losses=losses)
            if iou is not None:     # target, area, counts, input, pred, g_pred of the MaskIoU head, the mask loss gradient and the pooled features
                self.outputs.update(maskiou=iou, g_mask=g_mask, mask_pool=self.faster_rcnn.head.last_mask_pool, losses=losses)
            if pt is not None:      # coords, rois, input, pred, target, g_pred of the point head (backward adds g_in), the mask loss gradient
                self.outputs.update(point=pt, g_mask=g_mask, losses=losses)

    def _offset_of(self, prefix):
        cache = self.__dict__.setdefault('_offset_cache', {})
        if prefix not in cache:
            ps = self.faster_rcnn.ps
            cache[prefix] = min(o for name, (o, _) in ps.offsets.items() if name.startswith(prefix))
        return cache[prefix]
