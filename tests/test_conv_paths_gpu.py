"""GPU tests: every dispatch path of the convolution entry points against a float64 CPU reference, WITH THE PATH ASSERTED.

csrc/conv.hip picks, per pass and geometry, between un-split, split-K, tail-split and Winograd F(2x2) / F(4x4) launches, four GEMM tiles,
the 4-channel image-layer kernels and the operand arithmetic; the choice depends on the CU count, each kernel's occupancy and several
thresholds.  Every case here first asks the dispatcher itself (hnn.conv_plan -> mrcnn_conv2d_plan_query: the planning functions the
entry points call, nothing launched) which launch it gets and FAILS when that is not the one the case is named for - a change of a
threshold or of a kernel's occupancy can then no longer move a case onto another path silently.

Reference: torch CPU float64 (F.conv2d, F.conv_transpose2d, torch.nn.grad.conv2d_weight); error = max|got - ref| / max|ref|.
Bars (the ones tests/test_conv_gpu.py holds these kernels to): direct float32 forward 1e-5, backward-data / filter 2e-5, bias gradient
2e-5, Winograd F(2x2) 3e-5, F(4x4) 3e-4; arithmetic 3 (bf16x6): direct 2e-6, Winograd 3e-4.  Split-K / tail-split: the bar of the pass.
COLS_CASES: the 1x1 layer over the 9 C channels of a deformable layer's columns, K up to 4608, all three passes in both arithmetics."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from chainer_maskrcnn import _hip  # noqa: E402
from chainer_maskrcnn._hip import MrcnnHipError, nn as hnn  # noqa: E402
from test_conv_gpu import CASES, SPLIT_CASES, TAIL_SPLIT_LAYERS, TAIL_SPLIT_SIZES, _ref_conv  # noqa: E402

DEV = 'cuda:0'
FWD, BWD_DATA, BWD_FILTER = 0, 1, 2
DIRECT, SPLIT_K, TAIL_SPLIT, WINOGRAD = 0, 1, 2, 3
BIAS_TOL = 2e-5
WINO_TOL = {2: 3e-5, 4: 3e-4}


def direct_tol(pass_, arith):
    return 2e-6 if arith == 3 else (1e-5 if pass_ == FWD else 2e-5)


@contextlib.contextmanager
def settings(thresholds=(256, 2048, 0), pass_tiles=(2, 0, 0), split=(0, 0, 0), plan=(2, 2, 0)):
    """The process-global dispatch settings for the body, the library defaults afterwards."""
    lib = _hip.lib()
    try:
        _hip.check(lib.mrcnn_conv2d_set_winograd_thresholds(*thresholds))
        _hip.check(lib.mrcnn_conv2d_set_winograd_pass_tiles(*pass_tiles))
        _hip.check(lib.mrcnn_conv2d_set_split_operands(*split))
        _hip.check(lib.mrcnn_debug_conv_plan(*plan))
        _hip.check(lib.mrcnn_debug_conv_parts(0))
        yield
    finally:
        _hip.check(lib.mrcnn_conv2d_set_winograd_thresholds(256, 2048, 0))
        _hip.check(lib.mrcnn_conv2d_set_winograd_pass_tiles(2, 0, 0))
        _hip.check(lib.mrcnn_conv2d_set_split_operands(0, 0, 0))
        _hip.check(lib.mrcnn_debug_conv_plan(2, 2, 0))
        _hip.check(lib.mrcnn_debug_conv_parts(0))


def shapes(case):
    N, H, W, Cin, Cout, K, s, p = case
    return (N, H, W, Cin), (Cout, K, K, Cin)


def plan_of(pass_, case):
    xs, ws = shapes(case)
    return hnn.conv_plan(pass_, xs, ws, case[6], case[7])


def rel(got, ref):
    return (got.cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


class Layer:
    """Random operands of one layer (N, H, W, Cin, Cout, K, stride, pad), on the CPU and on the device, and its float64 results."""

    def __init__(self, case, seed, forward_only=False):
        N, H, W, Cin, Cout, K, s, p = self.case = case
        self.s, self.p = s, p
        g = torch.Generator().manual_seed(seed + sum(case))
        self.x = torch.randn((N, H, W, Cin), generator=g)
        self.w = torch.randn((Cout, K, K, Cin), generator=g) / (K * K * Cin) ** 0.5
        self.b = torch.randn((Cout,), generator=g)
        self._ref = {}
        if forward_only:                     # a case too large to keep the operands of the backward passes as well
            self.xd, self.wd, self.bd = (t.to(DEV) for t in (self.x, self.w, self.b))
            return
        Ho, Wo = hnn.conv_out(H, K, s, p), hnn.conv_out(W, K, s, p)
        self.gy = torch.randn((N, Ho, Wo, Cout), generator=g)
        self.base_x = torch.randn((N, H, W, Cin), generator=g)                    # what the accumulating calls add to
        self.base_w = torch.randn((Cout, K, K, Cin), generator=g)
        self.base_b = torch.randn((Cout,), generator=g)
        self.xr = torch.randn((N, H, W, Cin), generator=g).clamp_min(0)          # a ReLU output: the mask of relu_x
        self.xd, self.wd, self.bd, self.gyd, self.xrd = (t.to(DEV) for t in (self.x, self.w, self.b, self.gy, self.xr))
        self._ref = {}

    def ref_y(self, bias):
        if not bias and bias not in self._ref and True in self._ref:      # the bias is added last: one convolution serves both
            self._ref[bias] = self._ref[True] - self.b.double()
        if bias not in self._ref:
            self._ref[bias] = _ref_conv(self.x, self.w, self.b if bias else None, self.s, self.p)
        return self._ref[bias]

    def ref_gx(self):
        if 'gx' not in self._ref:
            self._ref['gx'] = F.conv_transpose2d(self.gy.permute(0, 3, 1, 2).double(), self.w.permute(0, 3, 1, 2).double(), None,
                                                 stride=self.s, padding=self.p).permute(0, 2, 3, 1).contiguous()
            assert self._ref['gx'].shape == self.x.shape
        return self._ref['gx']

    def ref_gw(self):
        if 'gw' not in self._ref:
            Cout, K, _, Cin = self.w.shape
            self._ref['gw'] = torch.nn.grad.conv2d_weight(self.x.double().permute(0, 3, 1, 2), (Cout, Cin, K, K), self.gy.double().permute(0, 3, 1, 2),
                                                          self.s, self.p).permute(0, 2, 3, 1).contiguous()
        return self._ref['gw']

    def ref_gb(self):
        return self.gy.double().sum((0, 1, 2))

    # ---- the three passes through the library, each variant against float64 ----
    def check_forward(self, tol, variants=((False, False), (True, False), (True, True))):
        for bias, relu in variants:
            ref = self.ref_y(bias).clamp_min(0) if relu else self.ref_y(bias)
            got = hnn.conv2d_fwd_raw(self.xd, self.wd, self.bd if bias else None, self.s, self.p, relu)
            assert got.shape == ref.shape
            err = rel(got, ref)
            print('fwd bias=%d relu=%d err %.2e' % (bias, relu, err))
            assert err < tol, ('fwd', bias, relu, err)

    def check_backward_data(self, tol):
        """plain, accumulate, relu_x, accumulate + relu_x (the mask applies to the TOTAL), and two calls give the same bits."""
        xs = tuple(self.x.shape)
        ref = self.ref_gx()
        mask = self.xr.double() > 0
        zero = torch.zeros_like(ref)
        for acc, relu_x in ((False, False), (True, False), (False, True), (True, True)):
            want = ref + self.base_x.double() if acc else ref
            if relu_x:
                want = torch.where(mask, want, zero)
            outs = []
            for _ in range(2):
                out = self.base_x.to(DEV).clone() if acc else None
                outs.append(hnn.conv2d_bwd_data_raw(self.gyd, self.wd, xs, self.s, self.p, out=out, relu_x=self.xrd if relu_x else None))
            assert torch.equal(outs[0], outs[1])
            err = rel(outs[0], want)
            print('bwd_data acc=%d relu_x=%d err %.2e' % (acc, relu_x, err))
            assert err < tol, ('bwd_data', acc, relu_x, err)
            if relu_x:
                assert (outs[0].cpu()[~mask] == 0).all()

    def check_backward_filter(self, tol):
        """overwrite with and without the bias gradient, and accumulate into non-zero gw / gb."""
        ws = tuple(self.w.shape)
        gw, gb = hnn.conv2d_bwd_filter_raw(self.xd, self.gyd, ws, self.s, self.p, True)
        gw2, gb2 = hnn.conv2d_bwd_filter_raw(self.xd, self.gyd, ws, self.s, self.p, True)
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
        gw3, none = hnn.conv2d_bwd_filter_raw(self.xd, self.gyd, ws, self.s, self.p, False)
        assert none is None and torch.equal(gw, gw3)
        acc_w, acc_b = self.base_w.to(DEV).clone(), self.base_b.to(DEV).clone()
        hnn.conv2d_bwd_filter_raw(self.xd, self.gyd, ws, self.s, self.p, True, gw=acc_w, gb=acc_b, accumulate=True)
        acc_w2, keep_b = self.base_w.to(DEV).clone(), self.base_b.to(DEV).clone()
        hnn.conv2d_bwd_filter_raw(self.xd, self.gyd, ws, self.s, self.p, False, gw=acc_w2, gb=keep_b, accumulate=True)
        assert torch.equal(acc_w, acc_w2) and torch.equal(keep_b.cpu(), self.base_b)        # no bias gradient asked: gb untouched
        errs = dict(gw=rel(gw, self.ref_gw()), gb=rel(gb, self.ref_gb()), acc_gw=rel(acc_w, self.ref_gw() + self.base_w.double()),
                    acc_gb=rel(acc_b, self.ref_gb() + self.base_b.double()))
        print('bwd_filter errs %s' % {k: '%.2e' % v for k, v in errs.items()})
        assert errs['gw'] < tol and errs['acc_gw'] < tol, errs
        assert errs['gb'] < BIAS_TOL and errs['acc_gb'] < BIAS_TOL, errs


# ---- the image layer ("stem"): Cin = 4, 7x7, stride 2, pad 3 - its own K-axis layout (tap, 4 channels) and fixed tiles -------------
# (1, 37, 45): 437 output pixels, fewer than the 512 two K chunks of the filter gradient need -> ksplit == 1; the other two: 874 and 768.
STEM_INPUTS = [(2, 37, 45), (1, 64, 48), (1, 37, 45)]
STEM_CASES = [(n, h, w, 4, cout, 7, 2, 3) for (n, h, w) in STEM_INPUTS for cout in (32, 64)]


def _stem_plans(case):
    pf, pw = plan_of(FWD, case), plan_of(BWD_FILTER, case)
    assert pf['smallc'] == 1 and pf['path'] == DIRECT and (pf['bm'], pf['bn']) == (128, 64) and pf['arithmetic'] == 0, pf
    assert pw['smallc'] == 1 and (pw['bm'], pw['bn']) == (64, 128) and pw['arithmetic'] == 0 and pw['wino_m'] == 0, pw
    return pf, pw


@pytest.mark.parametrize('case', STEM_CASES)
def test_stem_forward(case):
    with settings():
        _stem_plans(case)
        Layer(case, 11).check_forward(direct_tol(FWD, 0), variants=((False, False), (True, False), (False, True), (True, True)))


@pytest.mark.parametrize('case', STEM_CASES)
def test_stem_filter_gradient(case):
    N, H, W = case[:3]
    pixels = N * hnn.conv_out(H, 7, 2, 3) * hnn.conv_out(W, 7, 2, 3)
    with settings():
        _, pw = _stem_plans(case)
        if pixels < 512:
            assert pw['ksplit'] == 1 and pw['path'] == DIRECT, pw
        else:
            assert pw['ksplit'] > 1 and pw['path'] == SPLIT_K, pw
        Layer(case, 12).check_backward_filter(direct_tol(BWD_FILTER, 0))


def test_stem_filter_gradient_cases_cover_both_split_plans():
    px = [n * hnn.conv_out(h, 7, 2, 3) * hnn.conv_out(w, 7, 2, 3) for (n, h, w) in STEM_INPUTS]
    assert min(px) < 512 < max(px)
    with settings():
        ks = [plan_of(BWD_FILTER, c)['ksplit'] for c in STEM_CASES]
    assert min(ks) == 1 and max(ks) > 1, ks


@pytest.mark.parametrize('case', STEM_CASES[:2])
def test_stem_has_no_data_gradient(case):
    (N, H, W, _), ws = shapes(case)
    gy = torch.zeros((N, hnn.conv_out(H, 7, 2, 3), hnn.conv_out(W, 7, 2, 3), case[4]), device=DEV)
    with pytest.raises(MrcnnHipError):
        plan_of(BWD_DATA, case)
    with pytest.raises(MrcnnHipError):
        hnn.conv2d_bwd_data_raw(gy, torch.zeros(ws, device=DEV), (N, H, W, 4), 2, 3)
    with pytest.raises(MrcnnHipError):      # not only because of its stride
        hnn.conv2d_bwd_data_raw(torch.zeros((N, H, W, case[4]), device=DEV), torch.zeros(ws, device=DEV), (N, H, W, 4), 1, 3)


@pytest.mark.parametrize('case', STEM_CASES[:4])
def test_stem_ignores_split_operands(case):
    """The image layer has float32-MFMA kernels only: with split operands (3, 3, 3) set the query says arithmetic 0 and the results are
    bit-identical to the default's."""
    L = Layer(case, 13)
    ws = tuple(L.w.shape)
    outs = []
    for split in ((0, 0, 0), (3, 3, 3)):
        with settings(split=split):
            assert hnn.split_operands() == split
            _stem_plans(case)
            y = hnn.conv2d_fwd_raw(L.xd, L.wd, L.bd, 2, 3, True)
            gw, gb = hnn.conv2d_bwd_filter_raw(L.xd, L.gyd, ws, 2, 3, True)
            outs.append((y, gw, gb))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- strided layers, float32 MFMA and the shipped bf16x6 ------------------------------------------------------------------------------
STRIDED_CASES = [(2, 13, 9, 64, 96, 1, 2, 0),        # 1x1 stride 2 on odd maps
                 (1, 17, 21, 32, 64, 3, 2, 1)]       # 3x3 stride 2 pad 1


@pytest.mark.parametrize('arith', [0, 3])
@pytest.mark.parametrize('case', STRIDED_CASES)
def test_strided_forward_and_filter_gradient(case, arith):
    with settings(split=(arith,) * 3):
        for pass_ in (FWD, BWD_FILTER):
            pl = plan_of(pass_, case)
            assert pl['path'] == DIRECT and pl['smallc'] == 0 and pl['arithmetic'] == arith and pl['wino_m'] == 0, pl
        L = Layer(case, 21)
        L.check_forward(direct_tol(FWD, arith))
        L.check_backward_filter(direct_tol(BWD_FILTER, arith))


@pytest.mark.parametrize('case', STRIDED_CASES)
def test_strided_backward_data_is_declined(case):
    L = Layer(case, 22)
    with pytest.raises(MrcnnHipError):
        plan_of(BWD_DATA, case)
    with pytest.raises(MrcnnHipError):
        hnn.conv2d_bwd_data_raw(L.gyd, L.wd, tuple(L.x.shape), L.s, L.p)


# ---- float32 split-K in forward and backward-data (k_sum_slabs_ep: bias / ReLU / accumulate / ReLU-mask epilogues) ---------------------
SPLITK_CASES = [(2, 8, 8, 2048, 512, 1, 1, 0),       # few tiles, long K
                (1, 6, 6, 512, 64, 3, 1, 1)]         # 3x3, deep


def _fill_that_splits(pass_, case):
    """The default plan's fill, or the first larger one (the knob takes up to 16) under which the pass splits K."""
    lib = _hip.lib()
    for fill in range(2, 17):
        _hip.check(lib.mrcnn_debug_conv_plan(fill, 2, 0))
        pl = plan_of(pass_, case)
        if pl['path'] == SPLIT_K:
            assert pl['ksplit'] > 1 and pl['tail_ks'] == 0 and pl['arithmetic'] == 0 and pl['wino_m'] == 0, pl
            return fill
    pytest.fail('no fill up to 16 makes pass %d of %s a split-K launch: %s' % (pass_, case, pl))


@pytest.mark.parametrize('case', SPLITK_CASES)
def test_float32_split_k_forward(case):
    with settings():
        _fill_that_splits(FWD, case)
        L = Layer(case, 31)
        L.check_forward(direct_tol(FWD, 0), variants=((True, False), (True, True)))
        y = [hnn.conv2d_fwd_raw(L.xd, L.wd, L.bd, 1, case[7], True) for _ in range(2)]
        assert torch.equal(y[0], y[1])


@pytest.mark.parametrize('case', SPLITK_CASES)
def test_float32_split_k_backward_data(case):
    with settings():
        _fill_that_splits(BWD_DATA, case)
        Layer(case, 32).check_backward_data(direct_tol(BWD_DATA, 0))


# ---- the 1x1 layer over the 9 C channels of a deformable layer's columns, executed ----------------------------------
# K = 1152 / 2304 / 4608: the deepest GEMMs of the library.  The plan of a 1x1 layer depends on its pixel count alone - and on the chip: the
# tail split and the filter gradient's ksplit count workgroup slots with the occupancy the runtime reports for the kernel, which a host
# without a device replaces by 2 per CU, so the pixel counts below were found with the host-only query ON an MI355X (every count up to
# 2200 and 64 k, 64 k + 1 up to 89600) and are asserted there.  For every (width, pass, path) the section tabulates for the device the
# list holds the SMALLEST pixel count that takes that path, as a map of exactly that many pixels, and runs all three passes on it: one
# case serves several pairs.  A forward split-K and a direct backward-data launch start at one pixel; (1, 5, 7) stands beside (1, 1, 1)
# so that they also run on more than one row.  Filter gradient: the first split (512 pixels, two K chunks) and the largest ksplit of each
# width - 85 at 21760 pixels, 21 at 5376, 5 at 1280.  A forward tail split is on no line of the table; at K = 4608 it starts at 24577
# pixels (a 453 MB operand), where only the forward pass is run; at K = 2304 it starts at 49153 pixels and at K = 1152 beyond 89600:
# left out.  The float64 references of every other case take under a second on the CPU.
#   case, (forward, backward data, filter gradient) paths, ksplit of the filter gradient, the passes that are run
ALL3 = (FWD, BWD_DATA, BWD_FILTER)
COLS_CASES = [
    ((2, 16, 16, 1152, 128, 1, 1, 0), (SPLIT_K, DIRECT, SPLIT_K), 2, ALL3),                # res3, C = 128
    ((1, 3, 2731, 1152, 128, 1, 1, 0), (DIRECT, DIRECT, SPLIT_K), 29, ALL3),               # 8193 pixels: the first direct forward
    ((2, 85, 128, 1152, 128, 1, 1, 0), (DIRECT, DIRECT, SPLIT_K), 85, ALL3),               # 21760: the largest ksplit at this depth
    ((2, 16, 16, 2304, 256, 1, 1, 0), (SPLIT_K, DIRECT, SPLIT_K), 2, ALL3),                # res4, C = 256
    ((1, 17, 241, 2304, 256, 1, 1, 0), (DIRECT, DIRECT, SPLIT_K), 15, ALL3),               # 4097: the first direct forward
    ((2, 48, 56, 2304, 256, 1, 1, 0), (DIRECT, DIRECT, SPLIT_K), 21, ALL3),                # 5376: the largest ksplit
    ((1, 19, 283, 2304, 256, 1, 1, 0), (DIRECT, TAIL_SPLIT, SPLIT_K), 19, ALL3),           # 5377: the first tail-split backward data
    ((1, 1, 1, 4608, 512, 1, 1, 0), (SPLIT_K, SPLIT_K, DIRECT), 1, ALL3),                  # res5, C = 512
    ((1, 5, 7, 4608, 512, 1, 1, 0), (SPLIT_K, SPLIT_K, DIRECT), 1, ALL3),
    ((1, 1, 193, 4608, 512, 1, 1, 0), (SPLIT_K, DIRECT, DIRECT), 1, ALL3),                 # the first direct backward data
    ((2, 16, 16, 4608, 512, 1, 1, 0), (SPLIT_K, DIRECT, SPLIT_K), 2, ALL3),
    ((2, 20, 32, 4608, 512, 1, 1, 0), (SPLIT_K, DIRECT, SPLIT_K), 5, ALL3),                # 1280: the largest ksplit
    ((1, 3, 683, 4608, 512, 1, 1, 0), (DIRECT, DIRECT, SPLIT_K), 5, ALL3),                 # 2049: the first direct forward
    ((1, 1, 2689, 4608, 512, 1, 1, 0), (DIRECT, TAIL_SPLIT, SPLIT_K), 5, ALL3),            # the first tail-split backward data
    ((1, 7, 3511, 4608, 512, 1, 1, 0), (TAIL_SPLIT, TAIL_SPLIT, SPLIT_K), 5, (FWD,)),      # 24577: the first tail-split forward
]


@pytest.fixture(scope='module')
def cols_layer():
    """The operands and float64 results of one case, shared by its two arithmetics: one layer at a time, none after the last case."""
    kept = {}

    def get(case, passes):
        if case not in kept:
            kept.clear()
            kept[case] = Layer(case, 81, forward_only=passes == (FWD,))
        return kept[case]

    def release():
        kept.clear()
        torch.cuda.empty_cache()
    get.release = release
    yield get
    release()


def test_cols_cases_cover_the_table_of_the_deformable_layer():
    """Host only: widths 128 / 256 / 512 with K = 9 C; at K = 4608 direct, tail-split and split-K in forward and backward data and split-K
    in the filter gradient, each of them run; every pair DESIGN.md section 3.25 tabulates for the device; the largest ksplit of each width."""
    assert {(c[3], c[4]) for c, _, _, _ in COLS_CASES} == {(1152, 128), (2304, 256), (4608, 512)}
    run = {(c[4], pass_, paths[pass_]) for c, paths, _, passes in COLS_CASES for pass_ in passes}
    assert {(512, p, path) for p in (FWD, BWD_DATA) for path in (DIRECT, TAIL_SPLIT, SPLIT_K)} | {(512, BWD_FILTER, SPLIT_K)} <= run
    table = {(128, FWD, DIRECT), (128, BWD_DATA, DIRECT), (256, FWD, DIRECT), (256, BWD_DATA, DIRECT), (256, BWD_DATA, TAIL_SPLIT),
             (512, FWD, SPLIT_K), (512, FWD, DIRECT), (512, BWD_DATA, DIRECT)}
    assert table | {(C, BWD_FILTER, SPLIT_K) for C in (128, 256, 512)} <= run
    assert {C: max(ks for c, _, ks, _ in COLS_CASES if c[4] == C) for C in (128, 256, 512)} == {128: 85, 256: 21, 512: 5}


def _deep_forward(case, arith):
    """csrc/conv.hip deep_forward: under arithmetic 3 a forward launch of K >= 4096 never adds all of K in one accumulator."""
    return arith == 3 and case[3] * case[5] * case[5] >= 4096


@pytest.mark.parametrize('arith', [0, 3])          # (the inner loop: a case's two arithmetics share its layer)
@pytest.mark.parametrize('case,paths,ksplit,passes', COLS_CASES, ids=['x'.join(map(str, c[:4])) for c, _, _, _ in COLS_CASES])
def test_cols_layer_all_three_passes(case, paths, ksplit, passes, arith, cols_layer):
    """All three passes of every case, path asserted first.  The regression test of csrc/conv.hip's deep_forward rule: with all 144 K steps
    of K = 4608 in one float32 accumulator the un-split forward launch under arithmetic 3 measured 2.30e-06 at 2049 pixels and 2.92e-06 at
    2689 (without bias) against that arithmetic's bar of 2e-6 - the float32 MFMA measures 2.85e-06 / 3.17e-06 against its bar of 1e-5, and
    the same launch 1.2e-06 - 1.3e-06 at K = 1152 and 1.7e-06 - 1.8e-06 at K = 2304 -; in four parts of K it measures 1.02e-06 and 8.53e-07.
    The whole tiles of a tail split add up all of K as well (24577 pixels under the float32 MFMA: 2.88e-06 without bias), so under
    arithmetic 3 the rule takes that case too (8.19e-07); its three forward variants run in both arithmetics, the reference without
    bias being the one with bias minus the bias.
    The backward passes run first, so that a forward failure does not hide them."""
    with settings(split=(arith,) * 3):
        if _deep_forward(case, arith) and paths[FWD] != SPLIT_K:      # four parts of K instead of one sum, tail split or not
            paths = (SPLIT_K,) + paths[1:]
            assert plan_of(FWD, case)['ksplit'] == 4
        for pass_ in ALL3:
            pl = plan_of(pass_, case)
            assert pl['path'] == paths[pass_] and pl['arithmetic'] == arith and pl['wino_m'] == 0 and pl['smallc'] == 0, (pass_, pl)
            assert (pl['ksplit'] > 1) == (paths[pass_] == SPLIT_K) and (pl['tail_ks'] > 0) == (paths[pass_] == TAIL_SPLIT), (pass_, pl)
        assert pl['ksplit'] == ksplit, pl
        if paths[BWD_FILTER] == SPLIT_K:
            assert pl['ksplit'] > 1
        L = cols_layer(case, passes)
        try:
            if BWD_DATA in passes:
                L.check_backward_data(direct_tol(BWD_DATA, arith))
            if BWD_FILTER in passes:
                L.check_backward_filter(direct_tol(BWD_FILTER, arith))
            # the same three variants everywhere; with the bias first, Layer.ref_y takes the reference without it from that one
            L.check_forward(direct_tol(FWD, arith), variants=((True, False), (True, True), (False, False)))
        finally:
            if case == COLS_CASES[-1][0] and arith == 3:
                cols_layer.release()


# (case index, pass, the path from that pixel count on): one pixel fewer takes another path - the host-only query on the same chip
COLS_BOUNDARIES = [(1, FWD, DIRECT), (4, FWD, DIRECT), (6, BWD_DATA, TAIL_SPLIT), (9, BWD_DATA, DIRECT), (12, FWD, DIRECT),
                   (13, BWD_DATA, TAIL_SPLIT), (14, FWD, TAIL_SPLIT), (0, BWD_FILTER, SPLIT_K), (3, BWD_FILTER, SPLIT_K),
                   (10, BWD_FILTER, SPLIT_K)]


@pytest.mark.parametrize('index,pass_,path', COLS_BOUNDARIES)
def test_cols_cases_are_the_first_of_their_path(index, pass_, path):
    """Nothing launched: a case named the first of a path sits on the boundary - its pixel count takes the path, one pixel fewer does not."""
    case = COLS_CASES[index][0]
    pixels = case[0] * case[1] * case[2]
    with settings():
        assert plan_of(pass_, case)['path'] == path == COLS_CASES[index][1][pass_]
        assert plan_of(pass_, (1, 1, pixels - 1) + case[3:])['path'] != path
        assert plan_of(pass_, (1, 1, pixels) + case[3:])['path'] == path          # the count decides, not the map's shape


# ---- tail split on a small case found through the query --------------------------------------------------------------------------------
def _first_tail_split_height(pass_):
    """64 x 64 tiles forced, W = 64, 1x1 256 -> 256 (8 K steps, the fewest a tail split takes): the first H from 64 in steps of 8 whose grid
    ends a little past a whole number of rounds of workgroup slots.  Two images: the 64 x 64 kernels run 8 workgroups per CU on gfx950
    (2048 slots), and one image of at most 512 x 64 pixels has at most 2048 tiles of them - never more than one round."""
    for H in range(64, 513, 8):
        case = (2, H, 64, 256, 256, 1, 1, 0)
        pl = plan_of(pass_, case)
        if pl['tail_ks'] > 0:
            assert pl['path'] == TAIL_SPLIT and (pl['bm'], pl['bn']) == (64, 64) and pl['ksplit'] == 1, pl
            return case
    pytest.fail('no H in 64..512 takes the tail-split path in pass %d' % pass_)


def test_tail_split_forward_small():
    with settings(plan=(2, 2, 2)):
        L = Layer(_first_tail_split_height(FWD), 41)
        L.check_forward(direct_tol(FWD, 0), variants=((True, True),))


def test_tail_split_backward_data_small():
    with settings(plan=(2, 2, 2)):
        L = Layer(_first_tail_split_height(BWD_DATA), 42)
        L.check_backward_data(direct_tol(BWD_DATA, 0))


# ---- Winograd as shipped in the backward passes: F(4x4) from 64 channels, forward direct -------------------------------------------------
WINO_SHIPPED_CASES = [(2, 33, 37, 64, 96, 3, 1, 1), (1, 47, 61, 128, 64, 3, 1, 1)]      # odd maps, Cin != Cout, Cout below a 128 tile


@pytest.mark.parametrize('arith', [0, 3])
@pytest.mark.parametrize('case', WINO_SHIPPED_CASES)
def test_winograd_f4_backward_passes_as_shipped(case, arith):
    with settings(thresholds=(256, 2048, 0), pass_tiles=(2, 0, 0), split=(arith,) * 3):
        pf = plan_of(FWD, case)
        assert pf['path'] != WINOGRAD and pf['wino_m'] == 0 and pf['arithmetic'] == arith, pf
        for pass_ in (BWD_DATA, BWD_FILTER):
            pl = plan_of(pass_, case)
            assert pl['path'] == WINOGRAD and pl['wino_m'] == 4 and pl['arithmetic'] == arith, pl
        L = Layer(case, 51)
        L.check_forward(direct_tol(FWD, arith), variants=((True, True),))
        L.check_backward_data(WINO_TOL[4])
        L.check_backward_filter(WINO_TOL[4])


# ---- the automatic choice between F(2x2) and F(4x4) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,m', [((64, 6, 6, 256, 256, 3, 1, 1), 2),          # many tiny maps (RoI heads): 16 * 9 = 144 is not above 36 * 4 = 144
                                    ((16, 14, 14, 256, 256, 3, 1, 1), 4)])
def test_winograd_automatic_tile(case, m):
    with settings(thresholds=(256, 2048, 0), pass_tiles=(0, 0, 0)):
        for pass_ in (FWD, BWD_DATA, BWD_FILTER):
            pl = plan_of(pass_, case)
            assert pl['path'] == WINOGRAD and pl['wino_m'] == m and pl['arithmetic'] == 0, (pass_, pl)
        L = Layer(case, 61)
        L.check_forward(WINO_TOL[m])
        L.check_backward_data(WINO_TOL[m])
        L.check_backward_filter(WINO_TOL[m])


# ---- tile x pass census ---------------------------------------------------------------------------------------------------------------------
# The case that exists only to reach k_conv_igemm instantiations no other case list reaches (the census below): 128 x 128 tiles in the
# forward and backward-data kernels under arithmetic 3.
CENSUS_CASES = [      # case, (bm, bn) of forward, backward-data, filter gradient
    # 256 x 2 tiles of 128 x 128 = two workgroups for each of the 256 CUs: the fewest rows at which a 160-column GEMM takes that tile
    ((1, 181, 181, 160, 160, 1, 1, 0), ((128, 128), (128, 128), (128, 128))),
]
CENSUS_LAYERS = [c for c, _ in CENSUS_CASES]


@pytest.mark.parametrize('arith', [0, 3])
@pytest.mark.parametrize('case,tiles', CENSUS_CASES)
def test_census_cases_all_three_passes(case, tiles, arith):
    with settings(split=(arith,) * 3):
        for pass_ in (FWD, BWD_DATA, BWD_FILTER):
            pl = plan_of(pass_, case)
            assert pl['path'] != WINOGRAD and pl['smallc'] == 0 and pl['arithmetic'] == arith and (pl['bm'], pl['bn']) == tiles[pass_], (pass_, pl)
        L = Layer(case, 71)
        L.check_forward(direct_tol(FWD, arith))
        L.check_backward_data(direct_tol(BWD_DATA, arith))
        L.check_backward_filter(direct_tol(BWD_FILTER, arith))


def _visits():
    """(settings, case, passes) of every reference comparison of a convolution call in this file and in tests/test_conv_gpu.py."""
    v = []
    both = ((0, 0, 0), (3, 3, 3))
    all3 = (FWD, BWD_DATA, BWD_FILTER)
    for c in CASES:                                             # test_conv_forward, test_conv_backward_data_and_filter (stride 1)
        v.append((dict(), c, all3 if c[6] == 1 else (FWD,)))
    for c in SPLIT_CASES:                                       # test_conv_split_operands_all_three_passes, planes = 3
        N, H, W, Cin, Cout, K, p = c
        v.append((dict(pass_tiles=(0, 0, 0), split=(3, 3, 3)), (N, H, W, Cin, Cout, K, 1, p), all3))
    for c in STEM_CASES:
        v.append((dict(), c, (FWD, BWD_FILTER)))
    for split in both:
        for c in STRIDED_CASES:
            v.append((dict(split=split), c, (FWD, BWD_FILTER)))
        for c in WINO_SHIPPED_CASES:
            v.append((dict(split=split), c, all3))
        for c in CENSUS_LAYERS:
            v.append((dict(split=split), c, all3))
    for c in SPLITK_CASES:
        v.append((dict(), c, (FWD, BWD_DATA)))
    for (h, w) in TAIL_SPLIT_SIZES:                             # test_conv_tail_split_forward_and_backward_data
        for (k, cin, cout) in TAIL_SPLIT_LAYERS:
            v.append((dict(), (1, h, w, cin, cout, k, 1, k // 2), (FWD, BWD_DATA)))
    for c in ((64, 6, 6, 256, 256, 3, 1, 1), (16, 14, 14, 256, 256, 3, 1, 1)):
        v.append((dict(pass_tiles=(0, 0, 0)), c, all3))
    return v


def test_tile_pass_census():
    """Host only, nothing launched: over the case lists of this file and of tests/test_conv_gpu.py, under the settings their tests run
    them with, every k_conv_igemm instantiation the planner can choose is visited in arithmetic 0 and 3: (kernel mode, bm, bn) with the
    four tiles of choose_tile for forward and backward-data, the four of filter_tile for the filter gradient, and the two image-layer
    kernels.  A Winograd launch of the backward-data pass runs the FORWARD-kind GEMM, so it counts for the forward kernel; the
    persistent plane GEMM (256 x 256, its own kernels: tests/test_split_gemm_gpu.py) is listed and not counted."""
    seen, plane = {}, set()
    for kw, case, passes in _visits():
        with settings(**kw):
            for pass_ in passes:
                pl = plan_of(pass_, case)
                if pl['plane_gemm']:
                    plane.add((pass_, case))
                    continue
                mode = FWD if (pl['path'] == WINOGRAD and pass_ == BWD_DATA) else pass_
                seen.setdefault((mode, pl['bm'], pl['bn'], pl['arithmetic'], pl['smallc']), []).append((pass_, case))
    tiles = [(128, 128), (128, 64), (64, 128), (64, 64)]
    want = {(mode, bm, bn, arith, 0) for mode in (FWD, BWD_DATA, BWD_FILTER) for (bm, bn) in tiles for arith in (0, 3)}
    want |= {(FWD, 128, 64, 0, 1), (BWD_FILTER, 64, 128, 0, 1)}
    for k in sorted(seen):
        print(k, len(seen[k]), seen[k][0])
    print('plane GEMM launches:', sorted(plane))
    missing = sorted(want - set(seen))
    assert not missing, 'no case visits (kernel mode, bm, bn, arithmetic, smallc) = %s' % missing
    assert set(seen) <= want, sorted(set(seen) - want)
