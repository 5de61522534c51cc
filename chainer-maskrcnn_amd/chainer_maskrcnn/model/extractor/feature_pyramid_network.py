"""ResNet-50 + FPN feature extractor on gfx950 kernels.

Mirror of chainer_maskrcnn/model/extractor/feature_pyramid_network.py:9-71 (class attributes :9-16,
layers :22-40, forward :46-71) with the bottom-up network of Chainer's ``ResNet50Layers`` (SURVEY.md
Appendix A-8) spelled out.  Quirks kept on purpose (SURVEY.md Appendix B-1,2,4): 2x2/2 cover_all
max-pool after conv1, BatchNorm in training mode, no 3x3 smoothing on P5, P6 = 1x1 stride-2 conv of P5.
Tensors are NHWC; the image enters as (N,H,W,4) with a zero 4th channel.
"""
from chainer_maskrcnn.nn.core import Conv, BatchNorm, Bottleneck, MapGroupNorm, ParamStore
from chainer_maskrcnn._hip import ops, nn as hnn

# The ReLU backward of a bottleneck's output is applied by the kernels that WRITE that output's gradient (data-gradient epilogues,
# lattice scatter) instead of by the block's own bn3 backward: bn3's two backward kernels read two streams instead of three and the
# separate shortcut gradient is not written (same numbers bit for bit; False = the round-2 data flow, kept for A/B).
MASK_IN_PRODUCER = True
# Stream placement of the lateral 1x1 convolutions (OFF by default - built when the round's GPU minutes were spent,
# bit-identity and an A/B are in tests/test_step_gpu.py / tools/ab_step.py, the full suite has not run with it):
#   forward:  lat_p2 / lat_p3 / lat_p4 need c2 / c3 / c4 only - enqueued on the (idle) weight-gradient stream as soon as their ResNet stage
#             is done, they run beside the later stages instead of in the top-down chain;
#   backward: their data gradients g_c2 .. g_c4 are not needed until the matching ResNet stage - computed on a stream of their own, off the
#             chain conv_p2 -> conv_p3 -> conv_p4 -> toplayer -> res5.
# Same kernels, same operands, same summation order: the same bits.
# Ignored under fpn_norm='gn': each lateral's GroupNorm sits between it and the top-down add, and the laterals run on the chain.
LATERALS_OFF_THE_CHAIN = False
_lat_streams = {}


def _lateral_stream(device):
    import torch
    key = (device.type, device.index)
    if key not in _lat_streams:
        _lat_streams[key] = torch.cuda.Stream(device=device)
    return _lat_streams[key]


DCN_STAGES = ('res3', 'res4', 'res5')       # the stages dcn_stages may name


def dcn_stage_settings(dcn_stages=None, dcn_modulated=False):
    """The one statement of what dcn_stages / dcn_modulated may be: (the stages in network order - () when off,
    modulated).  ValueError for a stage other than DCN_STAGES or one named twice, and for ``dcn_modulated`` without stages."""
    if dcn_modulated not in (False, True, 0, 1):
        raise ValueError('dcn_modulated must be True or False, got %r' % (dcn_modulated,))
    if isinstance(dcn_stages, str):
        raise ValueError('dcn_stages must be a sequence of stage names, got %r' % (dcn_stages,))
    stages = tuple(dcn_stages or ())
    for s in stages:
        if s not in DCN_STAGES:
            raise ValueError('dcn_stages: unknown stage %r (one of %s)' % (s, ', '.join(DCN_STAGES)))
    if len(set(stages)) != len(stages):
        raise ValueError('dcn_stages names a stage twice: %r' % (stages,))
    if dcn_modulated and not stages:
        raise ValueError('dcn_modulated needs dcn_stages')
    return tuple(s for s in DCN_STAGES if s in stages), bool(dcn_modulated)


class FeaturePyramidNetwork(object):
    feat_strides = [4, 8, 16, 32, 64]
    spatial_scales = list(map(lambda x: 1. / x, feat_strides))
    anchor_base = 16
    anchor_sizes = [32, 64, 128, 256, 512]
    anchor_scales = list(map(lambda x: x / 16., anchor_sizes))

    STAGES = (('res2', 3, 64, 64, 256, 1), ('res3', 4, 256, 128, 512, 2),
              ('res4', 6, 512, 256, 1024, 2), ('res5', 3, 1024, 512, 2048, 2))

    def __init__(self, ps=None, prefix='extractor', stages=None, width_div=1, fpn_norm=None, gn_groups=32, dcn_stages=(), dcn_modulated=False):
        """``stages`` / ``width_div`` shrink the network for tests (blocks per stage, channel divisor);
        the defaults are the reference's ResNet-50.  fpn_norm: None = the reference's pyramid; 'gn' = a GroupNorm of ``gn_groups``
        groups (parameters ``<conv>/gn/gamma``, ``<conv>/gn/beta``) behind each of the eight FPN convolutions, which keep their bias
        (Detectron's *_gn configurations).  dcn_stages: the stages among 'res3', 'res4', 'res5' whose every block runs its
        3x3 layer as a deformable convolution, modulated (v2) with ``dcn_modulated`` (the dconv_c3-c5 / mdconv_c3-c5 configurations;
        parameters ``<block>/conv2_offset/{W,b}`` directly behind ``<block>/conv2/W``)."""
        self.dcn_stages, self.dcn_modulated = dcn_stage_settings(dcn_stages, dcn_modulated)
        if fpn_norm not in (None, 'gn'):
            raise ValueError("fpn_norm must be None or 'gn', got %r" % (fpn_norm,))
        if fpn_norm == 'gn' and (gn_groups < 1 or (256 // width_div) % gn_groups != 0):
            raise ValueError('gn_groups = %d does not divide the %d channels of the FPN' % (gn_groups, 256 // width_div))
        self.fpn_norm = fpn_norm
        self.ps = ps if ps is not None else ParamStore()
        p = prefix + '/'
        d = width_div
        self.conv1 = Conv(self.ps, p + 'resnet/conv1', 3, 64 // d, 7, 2, 3, bias=True, in_backbone=True)
        self.bn1 = BatchNorm(self.ps, p + 'resnet/bn1', 64 // d)
        self.stages = []
        for si, (name, n, cin, mid, cout, stride) in enumerate(self.STAGES):
            n = n if stages is None else stages[si]
            cin, mid, cout = cin // d, mid // d, cout // d
            deform = None if name not in self.dcn_stages else ('v2' if self.dcn_modulated else 'v1')
            blocks = [Bottleneck(self.ps, p + 'resnet/%s/a' % name, cin, mid, cout, stride, True, deform=deform)]
            for i in range(1, n):
                blocks.append(Bottleneck(self.ps, p + 'resnet/%s/b%d' % (name, i), cout, mid, cout, 1, False, deform=deform))
            self.stages.append(blocks)
        fc = 256 // d
        self.out_channels = fc
        self.norms = {}                 # convolution name -> its MapGroupNorm (empty without fpn_norm)

        def conv(name, *a, **kw):
            c = Conv(self.ps, p + name, *a, **kw)
            if fpn_norm == 'gn':        # registered directly behind its convolution: inside the FPN's range of the flat buffers
                self.norms[c.name] = MapGroupNorm(self.ps, c.name + '/gn', fc, gn_groups)
            return c
        self.toplayer = conv('toplayer', 2048 // d, fc, 1)
        self.conv_p4 = conv('conv_p4', fc, fc, 3, 1, 1, fwd_tile=0)
        self.conv_p3 = conv('conv_p3', fc, fc, 3, 1, 1, fwd_tile=0)
        self.conv_p2 = conv('conv_p2', fc, fc, 3, 1, 1, fwd_tile=0)
        self.conv_p6 = conv('conv_p6', fc, fc, 1, 2, 0)
        self.lat_p4 = conv('lat_p4', 1024 // d, fc, 1)
        self.lat_p3 = conv('lat_p3', 512 // d, fc, 1)
        self.lat_p2 = conv('lat_p2', 256 // d, fc, 1)
        self.anchor_scales = list(map(lambda x: x / float(self.anchor_base), self.anchor_sizes))
        self.freeze_bn, self.freeze_at = False, 0

    def set_freeze(self, bn=False, at=0):
        """bn: every BatchNorm of the ResNet runs the training step on its running statistics with a constant affine.
        at = k in 0..5: the stem (k >= 1) and the stages res2 .. res{k} are not trained - forward without a tape, no backward.
        Returns the names of the parameters this leaves constant (for ParamStore.set_frozen)."""
        at = int(at)
        if not 0 <= at <= 5:
            raise ValueError('freeze_at must be in 0..5 (0 = off, 1 = stem, k = stem + res2 .. res{k}), got %r' % (at,))
        if at > 0 and not bn:
            raise ValueError('freeze_at > 0 requires freeze_bn: a frozen prefix with batch-statistics BatchNorm is not implemented')
        self.freeze_bn, self.freeze_at = bool(bn), at
        self.bn1.frozen = bool(bn)
        names = set()
        for si, blocks in enumerate(self.stages):
            for b in blocks:
                b.trained = si + 2 > at
                for n in b.norms():
                    n.frozen = bool(bn)
        if bn:
            names.update(n for n in self.ps.offsets if '/resnet/' in n and (n.endswith('/gamma') or n.endswith('/beta')))
        for pre in self.frozen_prefixes():
            names.update(n for n in self.ps.offsets if n.startswith(pre + '/'))
        return names

    def frozen_prefixes(self):
        """Name prefixes of the layers freeze_at leaves untrained."""
        if self.freeze_at < 1:
            return []
        out = [self.conv1.name, self.bn1.name]
        for si in range(min(self.freeze_at - 1, len(self.stages))):
            out += [b.conv1.name.rsplit('/', 1)[0] for b in self.stages[si]]
        return out

    def __call__(self, x):
        """x (N,H,W,4) NHWC.  Returns (p2, p3, p4, p5, p6) NHWC and keeps the tape for backward()."""
        t = {}
        stem_trained = self.freeze_at < 1
        h, t['conv1'] = self.conv1.fwd(x, tape=stem_trained)
        h, t['bn1'] = self.bn1.fwd(h, relu=True)
        if stem_trained:
            t['pool_in'] = h
        else:
            t['bn1'] = None
        h = ops.maxpool2x2_fwd(h)
        cs = []
        t['blocks'] = []
        off_chain = self._laterals_off_chain(x)
        lat = {}
        if off_chain:
            import torch
            main, side = torch.cuda.current_stream(x.device), hnn.side_stream(x.device)
        for si, blocks in enumerate(self.stages):
            for b in blocks:
                h, ctx = b.fwd(h)
                if b.trained:                   # (a block of the frozen prefix leaves no tape)
                    t['blocks'].append((b, ctx))
            cs.append(h)
            if off_chain and si < 3:        # the stage's lateral, beside the stages that follow
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    lat[si] = (self.lat_p2, self.lat_p3, self.lat_p4)[si].fwd(h)
        c2, c3, c4, c5 = cs
        if off_chain:
            main.wait_stream(side)
            for l_, _ in lat.values():
                l_.record_stream(main)      # allocated on the side stream, consumed (and released) on the main stream
        return self.top_down(c2, c3, c4, c5, _tape=t, _lat=lat if off_chain else None)

    def _conv_fwd(self, conv, key, x, t, done=None):
        """conv (+ its GroupNorm under fpn_norm) on x; the contexts go to t[key] and t[key + '/gn'].  done: the convolution's (output,
        context) where it has already run (a lateral off the chain)."""
        y, t[key] = done if done is not None else conv.fwd(x)
        gn = self.norms.get(conv.name)
        if gn is not None:
            y, t[key + '/gn'] = gn.fwd(y)
        return y

    def _norm_bwd(self, conv, key, g):
        """The gradient of conv's output from the gradient of its GroupNorm's output (g itself without fpn_norm)."""
        gn = self.norms.get(conv.name)
        return g if gn is None else gn.bwd(self.tape[key + '/gn'], g)

    def top_down(self, c2, c3, c4, c5, _tape=None, _lat=None):
        """The pyramid from the four stage outputs: (p2, p3, p4, p5, p6) NHWC; keeps the tape for top_down_backward()."""
        t = {} if _tape is None else _tape
        lat = _lat or {}
        p5 = self._conv_fwd(self.toplayer, 'top', c5, t)
        l4 = self._conv_fwd(self.lat_p4, 'lat4', c4, t, lat.get(2))
        m4 = ops.upsample2x_add_fwd(p5, l4)
        p4 = self._conv_fwd(self.conv_p4, 'p4', m4, t)
        l3 = self._conv_fwd(self.lat_p3, 'lat3', c3, t, lat.get(1))
        m3 = ops.upsample2x_add_fwd(p4, l3)
        p3 = self._conv_fwd(self.conv_p3, 'p3', m3, t)
        l2 = self._conv_fwd(self.lat_p2, 'lat2', c2, t, lat.get(0))
        m2 = ops.upsample2x_add_fwd(p3, l2)
        p2 = self._conv_fwd(self.conv_p2, 'p2', m2, t)
        p6 = self._conv_fwd(self.conv_p6, 'p6', p5, t)
        self.tape = t
        return p2, p3, p4, p5, p6

    def _laterals_off_chain(self, t):
        return LATERALS_OFF_THE_CHAIN and self.fpn_norm is None and t.is_cuda and hnn.PROFILE is None

    def top_down_backward(self, grads):
        """grads: [g_p2, g_p3, g_p4, g_p5, g_p6]; consumed (accumulated into in place).  Returns (g_c2, g_c3, g_c4, g_c5), None where
        freeze_at leaves the stage below untrained.  Under fpn_norm each GroupNorm's backward runs in front of its convolution's;
        toplayer's runs last, when conv_p6, the upsampling and the caller have all added to g_p5."""
        t = self.tape
        g_p2, g_p3, g_p4, g_p5, g_p6 = grads
        self.conv_p6.bwd(t['p6'], self._norm_bwd(self.conv_p6, 'p6', g_p6), gx_acc=g_p5)
        g_m2 = self.conv_p2.bwd(t['p2'], self._norm_bwd(self.conv_p2, 'p2', g_p2))
        ops.upsample2x_bwd(g_m2, gtop=g_p3)
        # c2..c5 are ReLU outputs (the last block of a stage): every contribution to their gradient is masked where it is written
        # (mask_gx: data-gradient epilogue / lattice scatter), so the blocks' bn3 backward gets its gy with the mask applied
        off_chain = self._laterals_off_chain(g_p2)
        if off_chain:
            import torch
            main, ls = torch.cuda.current_stream(g_p2.device), _lateral_stream(g_p2.device)

        # freeze_at = k: the stages res2 .. res{k} take no gradient, so the 1x1 convolution that reads such a stage's output (lat_p2 for
        # k >= 2, ..., toplayer for k = 5) computes its filter gradient only
        k = self.freeze_at

        def lateral_bwd(conv, ctx, g_m, stage):
            if k >= stage:
                conv.bwd(ctx, g_m, need_gx=False)
                return None
            if not off_chain:
                return conv.bwd(ctx, g_m, mask_gx=MASK_IN_PRODUCER)
            ls.wait_stream(main)                # g_m is complete on the main stream
            g_m.record_stream(ls)
            with torch.cuda.stream(ls):         # (the filter gradient goes from here to the weight-gradient stream as everywhere)
                g_c = conv.bwd(ctx, g_m, mask_gx=MASK_IN_PRODUCER)
            g_c.record_stream(main)             # accumulated into by the next stage's first block, on the main stream
            return g_c
        g_c2 = lateral_bwd(self.lat_p2, t['lat2'], self._norm_bwd(self.lat_p2, 'lat2', g_m2), 2)
        g_m3 = self.conv_p3.bwd(t['p3'], self._norm_bwd(self.conv_p3, 'p3', g_p3))
        ops.upsample2x_bwd(g_m3, gtop=g_p4)
        g_c3 = lateral_bwd(self.lat_p3, t['lat3'], self._norm_bwd(self.lat_p3, 'lat3', g_m3), 3)
        g_m4 = self.conv_p4.bwd(t['p4'], self._norm_bwd(self.conv_p4, 'p4', g_p4))
        ops.upsample2x_bwd(g_m4, gtop=g_p5)
        g_c4 = lateral_bwd(self.lat_p4, t['lat4'], self._norm_bwd(self.lat_p4, 'lat4', g_m4), 4)
        # (freeze_at = 5: toplayer's filter gradient still needs its GroupNorm's backward)
        g_c5 = self.toplayer.bwd(t['top'], self._norm_bwd(self.toplayer, 'top', g_p5), need_gx=k < 5, mask_gx=MASK_IN_PRODUCER)
        return g_c2, g_c3, g_c4, g_c5

    def backward(self, grads, progress=None):
        """grads: [g_p2, g_p3, g_p4, g_p5, g_p6]; consumed (accumulated into in place).  ``progress(prefix)`` is
        called when every parameter registered at or after ``prefix`` has its final gradient (data-parallel overlap)."""
        t = self.tape
        k = self.freeze_at
        off_chain = self._laterals_off_chain(grads[0])
        if off_chain:
            import torch
            main, ls = torch.cuda.current_stream(grads[0].device), _lateral_stream(grads[0].device)
        g_c2, g_c3, g_c4, g_c5 = self.top_down_backward(grads)
        if progress:
            progress(self.toplayer.name)        # the FPN layers are registered after the ResNet
        # The gradient of c2..c4 is (lateral gradient) + (input gradient of the next stage): the next
        # stage's first block accumulates its input gradient into the lateral one (gx_acc).
        acc_for = {id(self.stages[k][0]): g for k, g in ((1, g_c2), (2, g_c3), (3, g_c4))}
        g = g_c5
        first = t['blocks'][0][0] if t['blocks'] else None
        for b, ctx in reversed(t['blocks']):
            # every block's output gradient arrives masked (from the block after it, or from toplayer / the laterals above); its own
            # input gradient is masked for the block before it - except the first block, whose input is the max-pool output
            if off_chain and acc_for.get(id(b)) is not None:
                main.wait_stream(ls)            # the lateral gradient this block accumulates into
            if k >= 1 and b is first:           # the first trained block above the frozen prefix: parameter gradients only
                g = b.bwd(ctx, g, gy_masked=MASK_IN_PRODUCER, need_gx=False)
            else:
                g = b.bwd(ctx, g, gx_acc=acc_for.get(id(b)), gy_masked=MASK_IN_PRODUCER, mask_gx=MASK_IN_PRODUCER and b is not first)
            if progress:
                progress(b.conv1.name)
        if k >= 1:
            # nothing below is trained; every prefix is still reported, in backward order, so that the data-parallel buckets and the
            # sectioned update close as without freezing (frozen parameters keep the zeros of their gradient slots)
            if progress:
                for blocks in reversed(self.stages[:k - 1]):
                    for b in reversed(blocks):
                        progress(b.conv1.name)
            self.tape = None
            return
        g = ops.maxpool2x2_bwd(t['pool_in'], g)
        g, _ = self.bn1.bwd(t['bn1'], g)
        self.conv1.bwd(t['conv1'], g, need_gx=False)
        self.tape = None
