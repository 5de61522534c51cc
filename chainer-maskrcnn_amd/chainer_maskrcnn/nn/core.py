"""Parameter store and layer objects with hand-written backward passes.

Role in the mirror of the reference: this is what Chainer's ``Link``/``Variable`` graph does for
chainer_maskrcnn/model/* - here as an explicit tape: ``y, ctx = layer.fwd(x)`` /
``gx = layer.bwd(ctx, gy)``.  All arithmetic is in csrc/*.hip; tensors are NHWC fp32 device
buffers.

MI355X-first choices
  * ONE flat fp32 buffer for all parameters, one for gradients, one for momentum: the optimiser is
    a single fused kernel and the data-parallel all-reduce runs over contiguous slices of the
    gradient buffer, launched bucket by bucket as backward produces them (parameters are registered
    in forward order, so backward fills the buffer from the end towards the start).
  * Fan-out points of the graph accumulate in place through the ``accumulate`` flags of the
    backward kernels instead of separate add passes.
"""
import math

import numpy as np
import torch

from chainer_maskrcnn._hip import nn as hnn
from chainer_maskrcnn._hip import ops


# chainer.config.train: BatchNorm uses batch statistics (True) or the running averages (False, MaskRCNN.predict).
TRAIN = True

# Weight-gradient GEMMs on a second stream (joined by join_side_stream() at the end of backward).
FILTER_GRAD_ON_SIDE_STREAM = True
# Winograd layers: one read of gy for the data gradient, the filter-gradient operand and the bias gradient.  Saves ~2 GB of
# reads per step but the filter gradient then starts after the data gradient (less overlap): same-box A/B 26.80 vs 26.68
# ms/step (tools/ab_step.py), so it is off.
WINOGRAD_SHARED_GY_TRANSFORM = False
# mask_rows='all': the backward pass of the mask branch leaves out the sampled rows the mask loss does not read (their gradient is an
# exact zero from the loss down to the pooled features) inside the kernels - same launches, same plans, same bits.
# False = the dense pass (tools/ab_step.py 'core.MASK_BWD_SKIP_INACTIVE=True' 'core.MASK_BWD_SKIP_INACTIVE=False').
MASK_BWD_SKIP_INACTIVE = True
# Per-layer Winograd tile of the FORWARD pass.  Measured on the full network (profiles/r02_winograd_layer_probe.txt): the
# F(4x4,3x3) forward transform costs gradient accuracy ONLY in the ResNet conv2 layers (their 1e-4 output error passes
# through training-mode BatchNorm and moves c4 / c5, hence the lateral / RPN gradients, by up to 2e-2); in the layers
# behind the backbone - FPN smoothing convolutions, the RPN convolution, the box / mask / keypoint head convolutions -
# every gradient stays at the float32 noise floor.  Those layers are built with fwd_tile=0 ("F(4x4) where the map is large
# enough"); while the process-wide forward setting is the shipped 2 their forward AND backward calls are bracketed with
# that value (the library reads the setting on the host at call time, and the filter-gradient pass reuses the forward's
# transformed input only when both used the same tile).  LAYER_TILE_HINTS = False: every layer follows the process-wide
# setting.  FWD_TILE_RULE: callable(layer name) -> tile or None, overrides the hints (measurement, tools/wino_error_probe.py).
LAYER_TILE_HINTS = True
FWD_TILE_RULE = None
# BatchNorm statistics from the producing convolution's GEMM epilogue (mrcnn_conv2d_fwd_bnstats_f32) where the launch allows
FUSE_BN_STATS = True
# Measurement (tests/tools/seed_table.py): with the float32-accurate emulation selected for the FORWARD pass, False keeps the forward
# pass of the layers behind the backbone (every convolution outside extractor/resnet: FPN, RPN, heads - no BatchNorm behind them) on the
# float32 MFMA.
FWD_EMULATION_BEHIND_BACKBONE = True
# ... and False here keeps the forward pass of the BACKBONE's convolutions (extractor/resnet) on the float32 MFMA.
FWD_EMULATION_IN_BACKBONE = True
# One foreign call per ResNet bottleneck and pass (csrc/blocks.hip: mrcnn_bottleneck_fwd_f32 / _bwd_f32 enqueue the block's whole chain of
# launches, same kernels / operands / order / streams as the per-layer path below - the same bits) instead of ~25 calls and ~20
# allocations: the host side of the step (train.py:117-132) was 16.4 ms of Python per 21.7 ms step (profiles/r04_host_time.txt).
# False = the per-layer path (also taken under bench instrumentation, evaluation mode and the measurement knobs it has no notion of).
COMPOSITE_BLOCKS = True


class _layer_tiles(object):
    def __init__(self, conv):
        self.t = FWD_TILE_RULE(conv.name) if FWD_TILE_RULE is not None else (conv.fwd_tile if LAYER_TILE_HINTS else None)
        self.keep = None
        self.behind = not conv.in_backbone                 # FPN laterals / smoothing, RPN, heads: no BatchNorm behind them

    def __enter__(self):
        self.keep_split = None
        if (not FWD_EMULATION_BEHIND_BACKBONE and self.behind) or (not FWD_EMULATION_IN_BACKBONE and not self.behind):
            sp = hnn.split_operands()
            if sp[0] == 3:
                self.keep_split = sp
                from chainer_maskrcnn._hip import lib, check
                check(lib().mrcnn_conv2d_set_split_operands(0, sp[1], sp[2]))
        if self.t is None:
            return
        cur = hnn.winograd_pass_tiles()
        if cur[0] == 2 and cur[0] != self.t:
            self.keep = cur
            hnn.set_winograd_pass_tiles(self.t, cur[1], cur[2])

    def __exit__(self, *a):
        if self.keep is not None:
            hnn.set_winograd_pass_tiles(*self.keep)
        if self.keep_split is not None:
            from chainer_maskrcnn._hip import lib, check
            check(lib().mrcnn_conv2d_set_split_operands(*self.keep_split))


def join_side_stream(device):
    torch.cuda.current_stream(device).wait_stream(hnn.side_stream(device))


def pad_to(n, m):
    return (n + m - 1) // m * m


class ParamStore(object):
    """Registers named parameters, then materialises them as views of flat device buffers."""

    ALIGN = 64          # floats (256 B): every view is 16-B aligned for the float4 kernels

    def __init__(self):
        self._specs = []        # (name, shape, init(np.RandomState) -> ndarray, trainable)
        self.offsets = {}
        self.params = self.grads = self.momentum = None
        self.size = 0
        self.buffers = {}       # non-trainable state (BN running statistics)
        self._views = {}        # id(flat buffer) -> (flat buffer, {name: view})
        self.frozen = frozenset()       # names the optimizer leaves alone (MaskRCNN.freeze) ...
        self.frozen_mask = None         # ... and their 64-float blocks, one bit each, on the parameters' device (None: nothing frozen)

    def register(self, name, shape, init, trainable=True):
        if name in self.offsets:
            raise KeyError('duplicate parameter %s' % name)
        n = int(np.prod(shape))
        if trainable:
            self.offsets[name] = (self.size, tuple(shape))
            self.size += pad_to(n, self.ALIGN)
        self._specs.append((name, tuple(shape), init, trainable))

    def materialise(self, device, seed=1234):
        rs = np.random.RandomState(seed)
        host = np.zeros((self.size,), np.float32)
        for name, shape, init, trainable in self._specs:
            v = np.asarray(init(rs), np.float32).reshape(shape)
            if trainable:
                o = self.offsets[name][0]
                host[o:o + v.size] = v.ravel()
            else:
                self.buffers[name] = torch.from_numpy(v.copy()).to(device)
        self.params = torch.from_numpy(host).to(device)
        self.grads = torch.zeros_like(self.params)
        self.momentum = torch.zeros_like(self.params)
        self._views = {}            # the views of earlier flat buffers (and the buffers they keep alive) go with them
        return self

    def frozen_block_mask(self, names):
        """One bit per ALIGN-float block of the flat buffers (bit b of word b // 32 = block b; int32 words on the host): set for
        the blocks of the parameters in ``names``.  Every parameter starts on a block boundary and owns whole blocks, its padding
        included, so a block is either frozen or trainable."""
        nblk = self.size // self.ALIGN
        bits = np.zeros((pad_to(max(nblk, 1), 32),), bool)
        for name in names:
            o, shape = self.offsets[name]
            bits[o // self.ALIGN:(o + pad_to(int(np.prod(shape)), self.ALIGN)) // self.ALIGN] = True
        words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view('<u4').reshape(-1)
        return torch.from_numpy(words.view(np.int32).copy())

    def set_frozen(self, names):
        """The optimizer updates every parameter except these (value, momentum and weight decay untouched); () = all trainable."""
        names = frozenset(names)
        for n in names:
            if n not in self.offsets:
                raise KeyError('no trainable parameter %s' % n)
        self.frozen = names
        self.frozen_mask = self.frozen_block_mask(names).to(self.params.device) if names else None

    def _view(self, flat, name):
        # (views are cached per flat buffer: ~250 parameter / gradient lookups per step were 1.6 ms of slicing)
        cache = self._views.get(id(flat))
        if cache is None or cache[0] is not flat:
            # a flat buffer this store no longer owns (rebound params / grads, a device move) must not stay alive through its views
            self._views = {k: c for k, c in self._views.items() if c[0] is self.params or c[0] is self.grads or c[0] is self.momentum}
            cache = self._views[id(flat)] = (flat, {})
        v = cache[1].get(name)
        if v is None:
            o, shape = self.offsets[name]
            v = cache[1][name] = flat[o:o + int(np.prod(shape))].view(shape)
        return v

    def p(self, name):
        return self._view(self.params, name)

    def g(self, name):
        return self._view(self.grads, name)

    def names(self):
        return list(self.offsets)

    def n_params(self):
        return sum(int(np.prod(s)) for _, s in self.offsets.values())


def lecun_normal(fan_in):
    return lambda shape: (lambda rs: rs.standard_normal(shape) * (1.0 / math.sqrt(fan_in)))


def normal(std):
    return lambda shape: (lambda rs: rs.standard_normal(shape) * std)


class Conv(object):
    """Convolution2D / Linear / (as 1x1 to 4*Cout) Deconvolution2D on NHWC tensors.

    Logical channel counts (cin, cout) are zero-padded to what the MFMA kernel wants (cin: multiple
    of 32, or 4 for the image layer; cout: multiple of 32).  ``cout_map`` optionally places logical
    output channels at chosen padded positions (fused heads).
    """

    def __init__(self, ps, name, cin, cout, k=1, stride=1, pad=0, bias=True, relu=False, init=None,
                 cin_p=None, cout_p=None, cout_index=None, fwd_tile=None, in_backbone=None):
        self.ps, self.name, self.fwd_tile = ps, name, fwd_tile
        # a convolution whose output feeds a training-mode BatchNorm (every backbone's: FPN ResNet, C4, Darknet, the res5 head) keeps its
        # FORWARD pass on the float32 MFMA under 'bf16x6_behind_backbone'; set by the extractor that builds it (default: by the FPN's names)
        self.in_backbone = ('/resnet/' in name) if in_backbone is None else bool(in_backbone)
        self.cin, self.cout, self.k, self.stride, self.pad, self.relu = cin, cout, k, stride, pad, relu
        self.cin_p = cin_p or (4 if cin <= 4 else pad_to(cin, 32))
        self.cout_p = cout_p or pad_to(cout, 32)
        self.has_bias = bias
        idx = np.arange(cout) if cout_index is None else np.asarray(cout_index)
        fan_in = cin * k * k
        gen = (init or lecun_normal(fan_in))((cout, k, k, cin))

        def w_init(rs):
            w = np.zeros((self.cout_p, k, k, self.cin_p), np.float32)
            w[idx, :, :, :cin] = gen(rs)
            return w
        ps.register(name + '/W', (self.cout_p, k, k, self.cin_p), w_init)
        if bias:
            ps.register(name + '/b', (self.cout_p,), lambda rs: np.zeros((self.cout_p,), np.float32))

    @property
    def W(self):
        return self.ps.p(self.name + '/W')

    @property
    def b(self):
        return self.ps.p(self.name + '/b') if self.has_bias else None

    @property
    def gW(self):
        return self.ps.g(self.name + '/W')

    def fwd(self, x, relu=None, bn_stats=False, tape=True):
        """bn_stats: the output feeds a training-mode BatchNorm - where the geometry allows, the GEMM epilogue also leaves the
        statistics partials in ``self.last_bn_part`` (None otherwise) and BatchNorm.fwd skips its statistics pass.
        tape=False: the layer is not trained (frozen backbone prefix) - nothing is kept for a backward pass, the context is None."""
        relu = self.relu if relu is None else relu
        self.last_bn_part = None
        hnn.LOGICAL = (self.cin, self.cout)
        if not tape:
            with _layer_tiles(self):
                y = hnn.conv2d_fwd_raw(x, self.W, self.b, self.stride, self.pad, relu)
            hnn.LOGICAL = None
            return y, None
        if bn_stats and FUSE_BN_STATS and TRAIN and not relu and not self.has_bias:
            with _layer_tiles(self):
                res = hnn.conv2d_fwd_bnstats_raw(x, self.W, self.stride, self.pad, keep_v=True)
            if res is not None:
                hnn.LOGICAL = None
                y, v, self.last_bn_part = res
                return y, (x, None, v)
        # training: layers on the Winograd path keep their transformed input for the filter-gradient pass
        with _layer_tiles(self):
            y, v = hnn.conv2d_fwd_raw(x, self.W, self.b, self.stride, self.pad, relu, keep_v=True) if TRAIN else \
                (hnn.conv2d_fwd_raw(x, self.W, self.b, self.stride, self.pad, relu), None)
        hnn.LOGICAL = None
        return y, (x, y if relu else None, v)

    def bwd(self, ctx, gy, need_gx=True, gx_acc=None, accumulate_params=False, gy_masked=False, mask_gx=False, active=None):
        """gy: gradient w.r.t. the (post-ReLU) output.  gx_acc: tensor to accumulate gx into.
        accumulate_params: add into the parameter gradients (layer applied several times).
        gy_masked: the producer of gy already applied this layer's ReLU mask (the layer above ran with mask_gx).
        mask_gx: this layer's input is itself a ReLU output - zero gx where x <= 0 in the data-gradient epilogue,
        which is the ReLU backward of the layer below (call that layer with gy_masked=True).
        active (uint8 (N,) or None): 0 = gy is all zero on that image (hnn.active_rows); forwarded to the two backward calls."""
        with _layer_tiles(self):
            return self._bwd(ctx, gy, need_gx, gx_acc, accumulate_params, gy_masked, mask_gx, active)

    def _bwd(self, ctx, gy, need_gx, gx_acc, accumulate_params, gy_masked, mask_gx, active=None):
        x, y, v = ctx
        if WINOGRAD_SHARED_GY_TRANSFORM:        # (the shared transform of gy feeds the dense GEMMs)
            active = None
        if y is not None and not gy_masked:
            gy = ops.relu_bwd(gy, y)
        gw = self.gW
        gb = self.ps.g(self.name + '/b') if self.has_bias else None
        hnn.LOGICAL = (self.cin, self.cout)
        try:
            if WINOGRAD_SHARED_GY_TRANSFORM and need_gx and self.stride == 1 and hnn.winograd_w_bytes(tuple(x.shape), tuple(gw.shape), 1, self.pad) > 0:
                # Winograd layer: the data-gradient call reads gy once for its own GEMM, the filter-gradient GEMM's
                # operand and the bias gradient; the filter gradient then runs on the side stream from the two kept
                # transforms (v from forward, wt from here) beside the next layer's backward
                assert not (mask_gx and gx_acc is not None)
                gx, wt = hnn.conv2d_bwd_data_raw(gy, self.W, tuple(x.shape), 1, self.pad, out=gx_acc, relu_x=x if mask_gx else None,
                                                 emit_w=True, gb=gb, gb_accumulate=accumulate_params)
                main = torch.cuda.current_stream(gy.device)
                side = hnn.side_stream(gy.device) if (FILTER_GRAD_ON_SIDE_STREAM and hnn.PROFILE is None) else main
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    hnn.conv2d_bwd_filter_raw(x, gy, tuple(gw.shape), 1, self.pad, False, gw=gw, gb=None,
                                              accumulate=accumulate_params, wino_v=v, wino_w=wt)
                if side is not main:
                    for t_ in (gy, x, v, wt):
                        if t_ is not None:
                            t_.record_stream(side)
                return gx
            if FILTER_GRAD_ON_SIDE_STREAM and hnn.PROFILE is None:
                main = torch.cuda.current_stream(gy.device)
                side = hnn.side_stream(gy.device)
                side.wait_stream(main)                      # gy (and x) are complete on the main stream
                with torch.cuda.stream(side):
                    hnn.conv2d_bwd_filter_raw(x, gy, tuple(gw.shape), self.stride, self.pad, self.has_bias, gw=gw, gb=gb,
                                              accumulate=accumulate_params, wino_v=v, active=active)
                gy.record_stream(side)                      # allocator: do not recycle gy before the side kernel is done
                x.record_stream(side)
                if v is not None:
                    v.record_stream(side)
                if active is not None:
                    active.record_stream(side)
            else:
                hnn.conv2d_bwd_filter_raw(x, gy, tuple(gw.shape), self.stride, self.pad, self.has_bias, gw=gw, gb=gb,
                                          accumulate=accumulate_params, wino_v=v, active=active)
            if not need_gx:
                return None
            if self.stride == 1:
                # (the epilogue masks the TOTAL: (old + product) where relu_x > 0 - direct, split-K and tail-split launches alike)
                assert not (mask_gx and gx_acc is not None) or self.k == 1
                return hnn.conv2d_bwd_data_raw(gy, self.W, tuple(x.shape), 1, self.pad, out=gx_acc,
                                               relu_x=x if mask_gx else None, active=active)
            if self.k > 1:
                # a strided k x k layer (the MaskIoU head's 3x3/2): the library's data gradient is stride 1 only, so gy is scattered onto
                # the stride-1 output lattice (zeros between) and that layer's data gradient is taken - the same sums plus zero terms
                assert self.k == 2 * self.pad + 1 and gx_acc is None, 'strided k x k backward-data: odd kernel with "same" padding'
                N, H, W, _ = x.shape
                g_up = ops.subsample_bwd(gy, (N, H, W, gy.shape[3]), self.stride)
                return hnn.conv2d_bwd_data_raw(g_up, self.W, tuple(x.shape), 1, self.pad, relu_x=x if mask_gx else None)
            assert self.pad == 0, 'strided backward-data of a 1x1 convolution takes no padding'
            g_sub = self.bwd_data_sub(gy)
        finally:
            hnn.LOGICAL = None
        return ops.subsample_bwd(g_sub, tuple(x.shape), self.stride, gx=gx_acc, relu_x=x if mask_gx else None)

    def bwd_data_sub(self, gy, out=None):
        """Data gradient of a strided 1x1 convolution on the subsampled lattice (N,Ho,Wo,Cin)."""
        N, Ho, Wo, _ = gy.shape
        keep = hnn.LOGICAL
        hnn.LOGICAL = (self.cin, self.cout)
        g = hnn.conv2d_bwd_data_raw(gy, self.W, (N, Ho, Wo, self.cin_p), 1, 0, out=out)
        hnn.LOGICAL = keep
        return g


class _ColsGemm(Conv):
    """The 1x1 layer a deformable convolution runs over its sampled columns: the (Cout,1,1,9*Cin) VIEW of the 3x3 filter (Cout,3,3,Cin) - the
    same memory, tap-major like the columns - and the same view of its gradient.  It registers nothing; every call goes through Conv's."""

    def __init__(self, conv):
        self.ps, self.name, self.fwd_tile, self.in_backbone = conv.ps, conv.name, None, conv.in_backbone
        self.cin, self.cout, self.k, self.stride, self.pad, self.relu = 9 * conv.cin, conv.cout, 1, 1, 0, False
        self.cin_p, self.cout_p, self.has_bias = 9 * conv.cin_p, conv.cout_p, False

    @property
    def W(self):
        return self.ps.p(self.name + '/W').view(self.cout_p, 1, 1, self.cin_p)

    @property
    def gW(self):
        return self.ps.g(self.name + '/W').view(self.cout_p, 1, 1, self.cin_p)


class DeformConv(Conv):
    """Deformable convolution (Dai et al. 2017; modulated=True: v2, Zhu et al. 2019) in place of a 3x3, stride 1, pad 1 layer without bias
    (DESIGN.md §3.25).  It owns the layer's ordinary parameters ``<name>/W`` (Cout,3,3,Cin) - registered as the plain layer registers them -
    and, directly behind them, an offset convolution ``<name>_offset/{W,b}``: 3x3, stride 1, pad 1, with a bias, 18 (v1) or 27 (v2) logical
    outputs, zero-initialised, so a fresh layer computes the plain convolution (v2: half of it, its masks being sigmoid(0)).
    Forward: the offset convolution on x, the sampled columns (N,H,W,9*Cin) (csrc/deform.hip), the library's convolution as a 1x1 layer over
    the columns.  The columns stay on the tape for the filter gradient.  No accuracy effect of the layer has been measured."""

    def __init__(self, ps, name, cin, cout, modulated=False, init=None, in_backbone=None):
        Conv.__init__(self, ps, name, cin, cout, 3, 1, 1, bias=False, init=init, in_backbone=in_backbone)
        self.modulated = bool(modulated)
        self.n_offset = 27 if self.modulated else 18
        zeros = lambda shape: (lambda rs: np.zeros(shape, np.float32))
        # (its output feeds no BatchNorm: not a backbone layer in the sense of Conv.in_backbone)
        self.offset = Conv(ps, name + '_offset', cin, self.n_offset, 3, 1, 1, bias=True, init=zeros, in_backbone=False)
        self.gemm = _ColsGemm(self)

    def fwd(self, x, relu=None, bn_stats=False, tape=True):
        """As Conv.fwd; the context is (x, offsets, the offset convolution's context, the 1x1 layer's context - which holds the columns)."""
        off, octx = self.offset.fwd(x, relu=False, tape=tape)
        cols = ops.deform_cols_fwd(x, off, self.modulated)
        y, gctx = self.gemm.fwd(cols, relu=self.relu if relu is None else relu, bn_stats=bn_stats, tape=tape)
        self.last_bn_part = self.gemm.last_bn_part
        return y, ((x, off, octx, gctx) if tape else None)

    def bwd(self, ctx, gy, need_gx=True, gx_acc=None, accumulate_params=False, gy_masked=False, mask_gx=False):
        """As Conv.bwd.  The filter gradient and the gradient of the columns are the 1x1 layer's; the offset (and mask) gradient goes through
        the offset convolution, whose data gradient and the sampling's input gradient are summed in one tensor (gx_acc when given), the ReLU
        mask of mask_gx applied once, to the total."""
        x, off, octx, gctx = ctx
        g_cols = self.gemm.bwd(gctx, gy, accumulate_params=accumulate_params, gy_masked=gy_masked)
        g_off = ops.deform_offset_bwd(g_cols, x, off, self.modulated)
        if not need_gx:
            self.offset.bwd(octx, g_off, need_gx=False, accumulate_params=accumulate_params)
            return None
        gx = self.offset.bwd(octx, g_off, gx_acc=gx_acc, accumulate_params=accumulate_params)
        return ops.deform_input_bwd(g_cols, off, self.modulated, tuple(x.shape), gx=gx, relu_x=x if mask_gx else None)


class BatchNorm(object):
    """Training-mode BatchNormalization (batch statistics; eps 2e-5, decay 0.9 as in Chainer).

    ``frozen`` (per layer, set by MaskRCNN.freeze): the training step runs the layer on its running statistics with a constant
    affine - the inference expression, bit for bit - and back-propagates through it as the per-channel scale it then is; no statistics,
    no gradient of gamma / beta, no update of avg_mean / avg_var."""

    def __init__(self, ps, name, c):
        self.ps, self.name, self.c = ps, name, c
        self.frozen = False
        ps.register(name + '/gamma', (c,), lambda rs: np.ones((c,), np.float32))
        ps.register(name + '/beta', (c,), lambda rs: np.zeros((c,), np.float32))
        ps.register(name + '/avg_mean', (c,), lambda rs: np.zeros((c,), np.float32), trainable=False)
        ps.register(name + '/avg_var', (c,), lambda rs: np.ones((c,), np.float32), trainable=False)

    def fwd(self, x, relu=False, residual=None, partials=None):
        gamma, beta = self.ps.p(self.name + '/gamma'), self.ps.p(self.name + '/beta')
        if not TRAIN or self.frozen:
            y = ops.bn_infer_fwd(x, gamma, beta, self.ps.buffers[self.name + '/avg_mean'], self.ps.buffers[self.name + '/avg_var'],
                                 residual, relu)
            if not TRAIN:
                return y, None
            # the ReLU mask is read from y: the layer's output is alive until the backward pass anyway (it is the next convolution's
            # operand), the convolution output x is not kept
            return y, ('frozen', y if relu else None)
        if partials is not None and partials.shape[2] == x.shape[-1]:
            y, mean, invstd = ops.bn_train_fwd_stats(x, partials, gamma, beta, residual, relu, self.ps.buffers[self.name + '/avg_mean'],
                                                     self.ps.buffers[self.name + '/avg_var'])
        else:
            y, mean, invstd = ops.bn_train_fwd(x, gamma, beta, residual, relu, self.ps.buffers[self.name + '/avg_mean'],
                                               self.ps.buffers[self.name + '/avg_var'])
        # BN + ReLU without a residual: backward recomputes the ReLU mask from x (bitwise the forward's y), so y is not
        # kept for (or read by) the backward pass
        return y, (x, y if (residual is not None or not relu) else None, mean, invstd, relu)

    def scale_operands(self):
        """(gamma, avg_var): what the frozen backward's per-channel scale gamma / sqrt(avg_var + eps) is made of."""
        return self.ps.p(self.name + '/gamma'), self.ps.buffers[self.name + '/avg_var']

    def bwd(self, ctx, gy, want_gres=False, gy_masked=False, in_place=False):
        """gy_masked: the producer of gy already zeroed it where this layer's ReLU output is <= 0 (its data-gradient epilogue
        ran with mask_gx on the tensor this layer produced): no mask stream is read here and gres would be gy itself.
        in_place (frozen layers): gx overwrites gy."""
        if ctx[0] == 'frozen':
            y = None if gy_masked else ctx[1]
            assert not (want_gres and y is None)
            gamma, var = self.scale_operands()
            return ops.bn_frozen_bwd(gy, gamma, var, yx=y, relu=0 if y is None else 1, want_gres=want_gres, out=gy if in_place else None)
        x, y, mean, invstd, relu = ctx
        if gy_masked:
            assert relu and not want_gres
            relu, y = False, None
        # the parameter gradients go straight into the flat gradient buffer
        gx, gres, _, _ = ops.bn_train_bwd(gy, x, y, self.ps.p(self.name + '/gamma'), mean, invstd, relu, want_gres,
                                          beta=self.ps.p(self.name + '/beta'), gg=self.ps.g(self.name + '/gamma'),
                                          gb=self.ps.g(self.name + '/beta'))
        return gx, gres


class GroupNorm(object):
    """GroupNorm (Wu & He 2018; eps 1e-5) of the RoI heads: ``c`` logical channels, zero-padded like the convolution above, in
    ``groups`` groups; statistics per RoI and group, the same in training and inference."""

    def __init__(self, ps, name, c, groups=32):
        if groups < 1 or c % groups != 0:
            raise ValueError('GroupNorm %s: %d groups do not divide %d channels' % (name, groups, c))
        self.ps, self.name, self.c, self.groups = ps, name, c, groups
        self.c_p = pad_to(c, 32)

        def ones(rs):
            g = np.zeros((self.c_p,), np.float32)
            g[:c] = 1.0
            return g
        ps.register(name + '/gamma', (self.c_p,), ones)
        ps.register(name + '/beta', (self.c_p,), lambda rs: np.zeros((self.c_p,), np.float32))

    def fwd(self, x, relu=False):
        """Returns (y, ctx); ctx = (x, mean, rstd, relu), None in evaluation mode (no statistics are kept).  y is not kept: the next
        layer's tape holds it."""
        gamma, beta = self.ps.p(self.name + '/gamma'), self.ps.p(self.name + '/beta')
        y, mean, rstd = ops.group_norm_fwd(x, gamma, beta, self.c, self.groups, relu=relu, want_stats=TRAIN)
        return y, ((x, mean, rstd, relu) if TRAIN else None)

    def bwd(self, ctx, gy, gy_masked=False, accumulate_params=False):
        """gy_masked: the producer of gy already zeroed it where this layer's ReLU output is <= 0 (its data-gradient epilogue ran with
        mask_gx on the tensor this layer produced); otherwise the mask of a ReLU layer is recomputed from x.  The parameter gradients go
        straight into the flat gradient buffer."""
        x, mean, rstd, relu = ctx
        gx, _, _ = ops.group_norm_bwd(gy, x, self.ps.p(self.name + '/gamma'), self.ps.p(self.name + '/beta'), mean, rstd, self.c,
                                      self.groups, relu=bool(relu) and not gy_masked, gg=self.ps.g(self.name + '/gamma'),
                                      gb=self.ps.g(self.name + '/beta'), accumulate_params=accumulate_params)
        return gx


class MapGroupNorm(GroupNorm):
    """GroupNorm behind a convolution of the FPN: the parameters and registration of GroupNorm, no ReLU.  Each call picks
    its kernels by host arithmetic on the shape: a map small enough for the register-resident kernels takes them; a larger one takes the
    split-reduction kernels of groupnorm_map.hip where they exist for the channel geometry, else the generic kernels."""

    def uses_map_path(self, shape):
        R, H, W, Cp = shape
        if ops.group_norm_plan(R, H, W, self.c, Cp, self.groups)[0] == 0:
            return False
        cpg = self.c // self.groups
        return cpg % 4 == 0 and cpg <= 256 and Cp <= 1024

    def fwd(self, x):
        """Returns (y, ctx); ctx = (x, mean, rstd), None in evaluation mode."""
        gamma, beta = self.ps.p(self.name + '/gamma'), self.ps.p(self.name + '/beta')
        if self.uses_map_path(x.shape):
            y, mean, rstd = ops.group_norm_map_fwd(x, gamma, beta, self.c, self.groups, want_stats=TRAIN)
        else:
            y, mean, rstd = ops.group_norm_fwd(x, gamma, beta, self.c, self.groups, relu=False, want_stats=TRAIN)
        return y, ((x, mean, rstd) if TRAIN else None)

    def bwd(self, ctx, gy, accumulate_params=False):
        """The parameter gradients go straight into the flat gradient buffer."""
        x, mean, rstd = ctx
        gamma, gg, gb = self.ps.p(self.name + '/gamma'), self.ps.g(self.name + '/gamma'), self.ps.g(self.name + '/beta')
        if self.uses_map_path(x.shape):
            return ops.group_norm_map_bwd(gy, x, gamma, mean, rstd, self.c, self.groups, gg=gg, gb=gb, accumulate_params=accumulate_params)[0]
        return ops.group_norm_bwd(gy, x, gamma, self.ps.p(self.name + '/beta'), mean, rstd, self.c, self.groups, relu=False, gg=gg, gb=gb,
                                  accumulate_params=accumulate_params)[0]


class Bottleneck(object):
    """ResNet bottleneck (Chainer BottleneckA when ``project`` else BottleneckB):
    relu(bn3(conv3(relu(bn2(conv2 3x3(relu(bn1(conv1 1x1/s))))))) + shortcut), stride on the first 1x1."""

    def __init__(self, ps, name, cin, mid, cout, stride, project, deform=None):
        """deform: None = the plain 3x3 conv2; 'v1' / 'v2' = a (modulated) deformable convolution in its place (DeformConv: the same
        ``conv2/W`` plus ``conv2_offset/{W,b}`` registered directly behind it).  A deformable block never takes the composite call."""
        if deform not in (None, 'v1', 'v2'):
            raise ValueError("deform must be None, 'v1' or 'v2', got %r" % (deform,))
        self.project, self.stride, self.deform = project, stride, deform
        he = lambda fan_in: (lambda shape: (lambda rs: rs.standard_normal(shape) * math.sqrt(2.0 / fan_in)))
        self.conv1 = Conv(ps, name + '/conv1', cin, mid, 1, stride, 0, bias=False, init=he(cin), in_backbone=True)
        self.bn1 = BatchNorm(ps, name + '/bn1', mid)
        if deform is None:
            self.conv2 = Conv(ps, name + '/conv2', mid, mid, 3, 1, 1, bias=False, init=he(mid * 9), in_backbone=True)
        else:
            self.conv2 = DeformConv(ps, name + '/conv2', mid, mid, modulated=deform == 'v2', init=he(mid * 9), in_backbone=True)
        self.bn2 = BatchNorm(ps, name + '/bn2', mid)
        self.conv3 = Conv(ps, name + '/conv3', mid, cout, 1, 1, 0, bias=False, init=he(mid), in_backbone=True)
        self.bn3 = BatchNorm(ps, name + '/bn3', cout)
        if project:
            self.conv4 = Conv(ps, name + '/conv4', cin, cout, 1, stride, 0, bias=False, init=he(cin), in_backbone=True)
            self.bn4 = BatchNorm(ps, name + '/bn4', cout)
        self.trained = True         # False: part of the frozen backbone prefix (MaskRCNN.freeze(at=...)) - forward only, no tape

    def norms(self):
        return [self.bn1, self.bn2, self.bn3] + ([self.bn4] if self.project else [])

    def _fwd_frozen(self, x):
        """Frozen BatchNorm (all of the block's layers): layer by layer on the running statistics, the projection pair in one apply.
        Neither the composite call nor conv2's bn1-on-load path exists for it (both are built on batch statistics)."""
        t = self.trained
        h1, c1 = self.conv1.fwd(x, tape=t)
        a1, b1 = self.bn1.fwd(h1, relu=True)
        h2, c2 = self.conv2.fwd(a1, tape=t)
        a2, b2 = self.bn2.fwd(h2, relu=True)
        h3, c3 = self.conv3.fwd(a2, tape=t)
        if self.project:
            h4, c4 = self.conv4.fwd(x, tape=t)
            ps, n3, n4 = self.bn3.ps, self.bn3.name, self.bn4.name
            y = ops.bn_infer_fwd_pair(h3, ps.p(n3 + '/gamma'), ps.p(n3 + '/beta'), ps.buffers[n3 + '/avg_mean'], ps.buffers[n3 + '/avg_var'],
                                      h4, ps.p(n4 + '/gamma'), ps.p(n4 + '/beta'), ps.buffers[n4 + '/avg_mean'], ps.buffers[n4 + '/avg_var'])
            b3 = ('frozen', y)
        else:
            c4 = None
            y, b3 = self.bn3.fwd(h3, relu=True, residual=x)
        if not t:
            return y, None
        return y, ('frozen', c1, b1, c2, b2, c3, b3, c4)

    def _bwd_frozen(self, ctx, gy, gx_acc, gy_masked, mask_gx, need_gx):
        """The frozen block's backward: every BatchNorm is a per-channel scale.  bn2 / bn1 get their gradient with the ReLU mask
        already applied by the convolution above them (mask_gx on its operand) and scale it in place."""
        _, c1, b1, c2, b2, c3, b3, c4 = ctx
        if self.project:
            g3, v3 = self.bn3.scale_operands()
            g4, v4 = self.bn4.scale_operands()
            g_h3, g_h4 = ops.bn_frozen_bwd_pair(gy, None if gy_masked else b3[1], g3, v3, g4, v4)
            g_r = None
        elif gy_masked:
            g_h3, _ = self.bn3.bwd(b3, gy, gy_masked=True)
            g_r = gy
        else:
            g_h3, g_r = self.bn3.bwd(b3, gy, want_gres=True)
        g_a2 = self.conv3.bwd(c3, g_h3, mask_gx=True)
        g_h2, _ = self.bn2.bwd(b2, g_a2, gy_masked=True, in_place=True)
        g_a1 = self.conv2.bwd(c2, g_h2, mask_gx=True)
        g_h1, _ = self.bn1.bwd(b1, g_a1, gy_masked=True, in_place=True)
        if not need_gx:         # the block below is frozen: filter gradients only
            self.conv1.bwd(c1, g_h1, need_gx=False)
            if self.project:
                self.conv4.bwd(c4, g_h4, need_gx=False)
            return None
        if not self.project:
            if gx_acc is not None:
                g_r = ops.add(g_r, gx_acc, out=gx_acc)
            return self.conv1.bwd(c1, g_h1, gx_acc=g_r, mask_gx=mask_gx)
        if self.stride == 1:
            gx = self.conv1.bwd(c1, g_h1, gx_acc=gx_acc)
            return self.conv4.bwd(c4, g_h4, gx_acc=gx, mask_gx=mask_gx)
        self.conv1.bwd(c1, g_h1, need_gx=False)
        self.conv4.bwd(c4, g_h4, need_gx=False)
        g_sub = self.conv1.bwd_data_sub(g_h1)
        self.conv4.bwd_data_sub(g_h4, out=g_sub)
        return ops.subsample_bwd(g_sub, tuple(c1[0].shape), self.stride, gx=gx_acc, relu_x=c1[0] if mask_gx else None)

    def _composite_ok(self, x):
        return (COMPOSITE_BLOCKS and TRAIN and FUSE_BN_STATS and x.is_cuda and hnn.PROFILE is None and FWD_TILE_RULE is None
                and not WINOGRAD_SHARED_GY_TRANSFORM and self.deform is None)

    def _descriptor(self, x):
        """mrcnn_bottleneck_t for this block on input x (cached: the parameter / gradient pointers are views of the flat buffers)."""
        ps = self.conv1.ps
        N, H, W, _ = x.shape
        fwd_split = -1 if FWD_EMULATION_IN_BACKBONE else 0
        # (every tensor whose raw pointer goes into the descriptor is part of the key: the BatchNorm running statistics live outside the
        # flat buffers and may be rebound on their own - ADVICE r5)
        bufs = tuple(ps.buffers[b.name + sfx].data_ptr() for b in ([self.bn1, self.bn2, self.bn3] + ([self.bn4] if self.project else []))
                     for sfx in ('/avg_mean', '/avg_var'))
        key = (N, H, W, ps.params.data_ptr(), ps.grads.data_ptr(), fwd_split, bufs)
        if getattr(self, '_desc_key', None) != key:
            from chainer_maskrcnn import _hip
            d = _hip.Bottleneck()
            d.N, d.H, d.W = N, H, W
            d.cin, d.mid, d.cout = self.conv1.cin_p, self.conv1.cout_p, self.conv3.cout_p
            d.stride, d.project, d.fwd_split = self.stride, int(self.project), fwd_split
            d.eps, d.decay = 2e-5, 0.9
            layers = [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)] + ([(self.conv4, self.bn4)] if self.project else [])
            for i, (c, b) in enumerate(layers):
                d.w[i], d.gw[i] = c.W.data_ptr(), ps.g(c.name + '/W').data_ptr()
                d.gamma[i], d.beta[i] = ps.p(b.name + '/gamma').data_ptr(), ps.p(b.name + '/beta').data_ptr()
                d.ggamma[i], d.gbeta[i] = ps.g(b.name + '/gamma').data_ptr(), ps.g(b.name + '/beta').data_ptr()
                d.run_mean[i], d.run_var[i] = ps.buffers[b.name + '/avg_mean'].data_ptr(), ps.buffers[b.name + '/avg_var'].data_ptr()
            self._desc, self._desc_key = d, key
        return self._desc

    def _fwd_composite(self, x):
        import ctypes
        from chainer_maskrcnn import _hip
        lib = _hip.lib()
        if not x.is_contiguous():
            raise ValueError('non-contiguous tensor passed to a HIP op')
        d = self._descriptor(x)
        plan = _hip.BottleneckPlan()
        _hip.check(lib.mrcnn_bottleneck_fwd_plan(ctypes.byref(d), ctypes.byref(plan)))
        N, H, W, _ = x.shape
        s = self.stride
        y = torch.empty((N, (H - 1) // s + 1, (W - 1) // s + 1, d.cout), dtype=torch.float32, device=x.device)
        arena = torch.empty((plan.arena_bytes,), dtype=torch.uint8, device=x.device)
        ws = hnn.workspace(plan.ws_bytes, x.device)
        _hip.check(lib.mrcnn_bottleneck_fwd_f32(ctypes.byref(d), ctypes.byref(plan), x.data_ptr(), y.data_ptr(), arena.data_ptr(), arena.numel(),
                                                ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
        return y, ('composite', x, y, arena, plan)

    def _bwd_composite(self, ctx, gy, gx_acc, gy_masked, mask_gx):
        import ctypes
        from chainer_maskrcnn import _hip
        lib = _hip.lib()
        _, x, y, fwd_arena, plan = ctx
        if not gy.is_contiguous() or (gx_acc is not None and not gx_acc.is_contiguous()):
            raise ValueError('non-contiguous tensor passed to a HIP op')
        d = self._descriptor(x)
        dev = x.device
        sizes = (ctypes.c_size_t * 3)()
        _hip.check(lib.mrcnn_bottleneck_bwd_sizes(ctypes.byref(d), sizes))
        main = torch.cuda.current_stream(dev)
        side = hnn.side_stream(dev) if FILTER_GRAD_ON_SIDE_STREAM else main
        arena = torch.empty((max(int(sizes[0]), 1),), dtype=torch.uint8, device=dev)
        ws_main, ws_side = hnn.workspace(sizes[1], dev, main), hnn.workspace(sizes[2], dev, side)
        g_r = None if (gy_masked or self.project) else torch.empty_like(y)      # (a projection block never writes the masked gradient)
        gx_new = torch.empty_like(x) if (self.project and gx_acc is None) else None
        _hip.check(lib.mrcnn_bottleneck_bwd_f32(ctypes.byref(d), ctypes.byref(plan), x.data_ptr(), y.data_ptr(), fwd_arena.data_ptr(), gy.data_ptr(),
                                                int(bool(gy_masked)), _hip.ptr(g_r), _hip.ptr(gx_acc), _hip.ptr(gx_new), int(bool(mask_gx)),
                                                arena.data_ptr(), arena.numel(), ws_main.data_ptr(), ws_main.numel(), ws_side.data_ptr(),
                                                ws_side.numel(), main.cuda_stream, side.cuda_stream))
        if side is not main:            # the filter gradients read these on the side stream: the allocator must not recycle them before
            for t_ in (x, fwd_arena, arena):
                t_.record_stream(side)
        if gx_acc is not None:
            return gx_acc
        if self.project:
            return gx_new
        return gy if gy_masked else g_r          # identity shortcut: accumulated into the shortcut gradient in place

    def fwd(self, x):
        if TRAIN and self.bn1.frozen:
            return self._fwd_frozen(x)
        if self._composite_ok(x):
            return self._fwd_composite(x)
        h1, c1 = self.conv1.fwd(x, bn_stats=True)
        a1, b1 = self.bn1.fwd(h1, relu=True, partials=self.conv1.last_bn_part)
        h2, c2 = self.conv2.fwd(a1, bn_stats=True)
        a2, b2 = self.bn2.fwd(h2, relu=True, partials=self.conv2.last_bn_part)
        h3, c3 = self.conv3.fwd(a2, bn_stats=True)
        p3 = self.conv3.last_bn_part
        if self.project:
            h4, c4 = self.conv4.fwd(x, bn_stats=True)
            r, b4 = self.bn4.fwd(h4, partials=self.conv4.last_bn_part)
        else:
            r, c4, b4 = x, None, None
        y, b3 = self.bn3.fwd(h3, relu=True, residual=r, partials=p3)
        return y, (c1, b1, c2, b2, c3, b3, c4, b4)

    def bwd(self, ctx, gy, gx_acc=None, gy_masked=False, mask_gx=False, need_gx=True):
        """need_gx=False (frozen blocks only: the first trained block above a frozen prefix): parameter gradients only, returns None.
        gy_masked: gy already carries this block's output ReLU mask (its producer ran with mask_gx on this block's output);
        bn3's backward then reads two streams instead of three and writes no separate shortcut gradient (it IS gy).
        mask_gx: the block's input is itself a ReLU output (the previous block's): the returned gradient - the sum of all its
        contributions - is zeroed where that input is <= 0, in the epilogue of the kernel that writes it last."""
        if ctx[0] == 'frozen':
            return self._bwd_frozen(ctx, gy, gx_acc, gy_masked, mask_gx, need_gx)
        assert need_gx, 'need_gx=False exists for blocks with frozen BatchNorm only'
        if ctx[0] == 'composite':
            return self._bwd_composite(ctx, gy, gx_acc, gy_masked, mask_gx)
        c1, b1, c2, b2, c3, b3, c4, b4 = ctx
        if gy_masked:
            g_h3, _ = self.bn3.bwd(b3, gy, gy_masked=True)
            g_r = gy
        else:
            g_h3, g_r = self.bn3.bwd(b3, gy, want_gres=True)
        g_a2 = self.conv3.bwd(c3, g_h3)
        g_h2, _ = self.bn2.bwd(b2, g_a2)
        g_a1 = self.conv2.bwd(c2, g_h2)
        g_h1, _ = self.bn1.bwd(b1, g_a1)
        if not self.project:
            if gx_acc is not None:
                g_r = ops.add(g_r, gx_acc, out=gx_acc)
            return self.conv1.bwd(c1, g_h1, gx_acc=g_r, mask_gx=mask_gx)
        g_h4, _ = self.bn4.bwd(b4, g_r)
        if self.stride == 1:
            gx = self.conv1.bwd(c1, g_h1, gx_acc=gx_acc)
            return self.conv4.bwd(c4, g_h4, gx_acc=gx, mask_gx=mask_gx)
        # both strided 1x1 convolutions read the same lattice: sum on the lattice, scatter once
        self.conv1.bwd(c1, g_h1, need_gx=False)
        self.conv4.bwd(c4, g_h4, need_gx=False)
        g_sub = self.conv1.bwd_data_sub(g_h1)
        self.conv4.bwd_data_sub(g_h4, out=g_sub)
        return ops.subsample_bwd(g_sub, tuple(c1[0].shape), self.stride, gx=gx_acc, relu_x=c1[0] if mask_gx else None)
