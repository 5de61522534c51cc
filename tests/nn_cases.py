"""The plan-edge cases of csrc/nn.hip's BatchNorm reductions and their float64 references (NumPy only: no GPU, no torch device).

`red_plan` restates the library's reduction plan (nn.hip red_plan; tests/test_nn_plan_gpu.py checks it against mrcnn_bn_workspace_bytes for
every case), `thread_rows` the number of rows one thread of one block sums under that plan.  The tables name, per case, the edge it
exists for; tests/test_nn_cases_cpu.py checks by the restated plan that each case reaches it."""
import collections

import numpy as np

NT = 256                    # threads of a reduction block
SHIPPED_CAP = 1024          # g_red_cap
EPS, DECAY = 2e-5, 0.9

# what the issue asks the table to reach
STATS_ROWS = (0, 1, 3, 4, 5, 7, 8, 9)       # k_bn_stats_partial: four rows in flight, then a tail
BWD_ROWS = (0, 1, 2, 3)                     # k_bn_bwd_partial / k_bn_bwd_partial2: two rows in flight, then a tail
NBLK = (1, 2, 63, 64, 65, 255, 256, 257)    # reduce_partials: 64 or 256 slices, four partial rows in flight, then a tail
PLAN_C = (4, 8, 16, 64, 256, 1024, 2048)


def red_plan(P, C, red_cap=SHIPPED_CAP):
    """(G, RPI, nblk, rows_per_blk) of nn.hip red_plan."""
    C4 = C // 4
    G = min(C4, NT)
    RPI = NT // G
    want = (P * C4 + NT * 16 - 1) // (NT * 16)
    nblk = max(1, min(want, red_cap))
    rpb = (P + nblk - 1) // nblk
    rpb = (rpb + RPI - 1) // RPI * RPI
    nblk = (P + rpb - 1) // rpb
    return G, RPI, nblk, rpb


def block_rows(P, C, red_cap=SHIPPED_CAP):
    """Rows of each block, first to last."""
    _, _, nblk, rpb = red_plan(P, C, red_cap)
    return [min(P, (b + 1) * rpb) - b * rpb for b in range(nblk)]


def thread_rows(P, C, red_cap=SHIPPED_CAP):
    """The set of row counts one thread (row lane rr < RPI) of one block sums: rows rr, rr + RPI, ... of the block's rows."""
    _, RPI, _, _ = red_plan(P, C, red_cap)
    out = set()
    for n in set(block_rows(P, C, red_cap)):
        for rr in range(RPI):
            out.add(max(0, (n - rr + RPI - 1) // RPI))
    return out


def workspace_bytes(P, C, red_cap=SHIPPED_CAP, stats=2):
    return red_plan(P, C, red_cap)[2] * stats * C * 4


def channels_refused(C):
    """C / 4 above 256 and no multiple of 256: the reduction passes' channel loop would run a different number of barrier trips per
    thread; the entry points refuse it."""
    return C // 4 > NT and (C // 4) % NT != 0


# ---- the plan cases ------------------------------------------------------------------------------------------------------------------
# edges: ('rows', k) a thread of some block sums k rows; ('nblk', n); ('P', p); 'P<RPI'; 'single_row_tail' (the last block has one row);
# 'cap_binds' (red_cap, not the size, sets the block count).  big: more than 2^19 elements (the natural sizes of the large block counts).
PlanCase = collections.namedtuple('PlanCase', 'name P C red_cap edges')


def _pc(P, C, cap, *edges):
    return PlanCase('P%d_C%d_cap%d' % (P, C, cap), P, C, cap, edges)


def _rows(*ks):
    return tuple(('rows', k) for k in ks)


PLAN_CASES = [
    # C = 4: G = 1, RPI = 256
    _pc(1, 4, 1024, ('P', 1), 'P<RPI', *_rows(0, 1)),
    _pc(513, 4, 1024, *_rows(2, 3)),
    _pc(1025, 4, 1024, *_rows(4, 5)),
    _pc(1793, 4, 1024, *_rows(7, 8)),
    _pc(2049, 4, 1024, *_rows(8, 9)),
    # C = 8: G = 2, RPI = 128
    _pc(2, 8, 1024, ('P', 2), 'P<RPI', *_rows(0, 1)),
    _pc(257, 8, 1024, *_rows(2, 3)),
    _pc(513, 8, 1024, *_rows(4, 5)),
    _pc(897, 8, 1024, *_rows(7, 8)),
    _pc(1025, 8, 1024, *_rows(8, 9)),
    # C = 16: G = 4, RPI = 64
    _pc(3, 16, 1024, ('P', 3), 'P<RPI', *_rows(0, 1)),
    _pc(129, 16, 1024, *_rows(2, 3)),
    _pc(257, 16, 1024, *_rows(4, 5)),
    _pc(449, 16, 1024, *_rows(7, 8)),
    _pc(513, 16, 1024, *_rows(8, 9)),
    # C = 64: G = 16, RPI = 16
    _pc(1, 64, 1024, ('P', 1), 'P<RPI', *_rows(0, 1)),
    _pc(33, 64, 1024, *_rows(2, 3)),
    _pc(65, 64, 1024, *_rows(4, 5)),
    _pc(113, 64, 1024, *_rows(7, 8)),
    _pc(129, 64, 1024, *_rows(8, 9)),
    # C = 256: G = 64, RPI = 4
    _pc(3, 256, 1024, ('P', 3), 'P<RPI', *_rows(0, 1)),
    _pc(9, 256, 1024, *_rows(2, 3)),
    _pc(17, 256, 1024, *_rows(4, 5)),
    _pc(29, 256, 1024, *_rows(7, 8)),
    _pc(33, 256, 1024, *_rows(8, 9)),
    # C = 1024: G = 256, RPI = 1: a thread's rows are its block's rows (never 0); one block up to P = 16
    _pc(1, 1024, 1024, ('P', 1), *_rows(1)),
    _pc(2, 1024, 1024, ('P', 2), *_rows(2)),
    _pc(3, 1024, 1024, ('P', 3), *_rows(3)),
    _pc(4, 1024, 1024, *_rows(4)),
    _pc(5, 1024, 1024, *_rows(5)),
    _pc(7, 1024, 1024, *_rows(7)),
    _pc(17, 1024, 1024, ('nblk', 2), *_rows(8, 9)),
    # C = 2048: G = 256, RPI = 1, two trips of the channel loop; one block up to P = 8
    _pc(1, 2048, 1024, ('P', 1), ('nblk', 1), *_rows(1)),
    _pc(2, 2048, 1024, ('P', 2), *_rows(2)),
    _pc(3, 2048, 1024, ('P', 3), *_rows(3)),
    _pc(9, 2048, 1024, ('nblk', 2), *_rows(4, 5)),
    _pc(15, 2048, 1024, ('nblk', 2), *_rows(7, 8)),
    _pc(17, 2048, 2, 'cap_binds', ('nblk', 2), *_rows(8, 9)),
    _pc(25, 2048, 3, 'cap_binds', ('nblk', 3), *_rows(7, 9)),
    _pc(57, 2048, 1024, 'single_row_tail', *_rows(1, 8)),
    # a last block with a single row behind full blocks, RPI > 1
    _pc(15 * 256 + 1, 64, 1024, 'single_row_tail'),
    # the block counts at the finaliser's slice edges (natural sizes, the cap set to the count)
    _pc(63 * 8, 2048, 63, ('nblk', 63)),
    _pc(64 * 8, 2048, 64, ('nblk', 64)),
    _pc(65 * 8, 2048, 65, ('nblk', 65)),
    _pc(255 * 8, 2048, 255, ('nblk', 255)),
    _pc(256 * 8, 2048, 256, ('nblk', 256)),
    _pc(257 * 8, 2048, 257, ('nblk', 257)),
    _pc(256 * 256 + 1, 64, 1024, ('nblk', 257), 'single_row_tail'),
]


def plan_data(case, seed_offset=0):
    """Float32 inputs of a plan case: x with |mean| > std, gamma, beta, a residual, gy and a second tensor for the pair."""
    rs = np.random.RandomState(1000 + case.P + 7 * case.C + case.red_cap + seed_offset)
    P, C = case.P, case.C
    f = np.float32
    return dict(x=(rs.standard_normal((P, C)) * 2 + 3).astype(f), xb=(rs.standard_normal((P, C)) * 0.7 - 1).astype(f),
                gamma=rs.uniform(0.5, 1.5, C).astype(f), beta=rs.standard_normal(C).astype(f),
                gamma_b=rs.uniform(0.5, 1.5, C).astype(f), beta_b=(rs.standard_normal(C) * 0.1).astype(f),
                res=rs.standard_normal((P, C)).astype(f), gy=rs.standard_normal((P, C)).astype(f))


# ---- hand-made epilogue partials -------------------------------------------------------------------------------------------------------
# (rows, C): reduce_partials at its slice edges, the channel blocks partly outside for C = 4, 8, 20; |mean| / std ~ 1.5: no recompute
PARTIAL_CASES = [(1, 4), (63, 8), (64, 20), (65, 64), (255, 4), (256, 64), (257, 20), (1024, 8), (1024, 64), (65, 20)]
PARTIAL_P = 2051

# (P, ratio, C, only_one): the exact recompute of k_bn_stats_final (eight rows in flight per slice, FIN_SLICES = 16 / 64, then a tail) at
# its edges; only_one: one channel of each 16-channel block has |mean| / std = ratio, the others 1.5.  C = 20: lanes with c >= C.
RECOMPUTE_CASES = [(1, 80.0, 64, False), (15, 20.0, 64, False), (16, 80.0, 20, False), (17, 400.0, 64, False), (127, 80.0, 20, False),
                   (128, 400.0, 64, False), (129, 20.0, 64, False), (129, 80.0, 64, True), (1000, 400.0, 20, False), (1000, 80.0, 64, True),
                   (1000, 20.0, 64, False)]


def large_mean_data(P, ratio, C, only_one, seed=5):
    """x (P, C) float32 with unit standard deviation and |mean| = ratio per channel (only_one: channel 5 of every 16 only, 1.5 elsewhere)."""
    rs = np.random.RandomState(seed + P + C)
    m = np.full(C, ratio)
    if only_one:
        m[:] = 1.5
        m[5::16] = ratio
    m *= np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    return (rs.standard_normal((P, C)) + m).astype(np.float32)


def make_partials(x, rows):
    """part (rows, 2, C): un-shifted float32 sums and sums of squares of a split of x's rows into `rows` runs (runs may be empty), each
    the correctly rounded float32 value of the run's sum: the best the format can hold, so that a test of the finaliser sees the
    finaliser's error and not the builder's (at |mean| / std = 20 a few ulps on a run's sums already cost 2e-5 of 1 / sigma)."""
    P, C = x.shape
    part = np.zeros((rows, 2, C), np.float32)
    edges = [(k * P) // rows for k in range(rows + 1)]
    x64 = x.astype(np.float64)
    for k in range(rows):
        blk = x64[edges[k]:edges[k + 1]]
        if len(blk):
            part[k, 0] = blk.sum(0).astype(np.float32)
            part[k, 1] = (blk * blk).sum(0).astype(np.float32)
    return part


def recompute_rows(P):
    """Partial rows of a recompute case: one row per run, so the partials hold x exactly and x^2 to half an ulp.  A float32 run sum of
    n values at |mean| / std = r is off by up to eps32 / 2 of n r std (sums) and n r^2 std^2 (squares), which the variance P std^2 sees
    r^2 times enlarged: runs of 4 rows at P = 15, r = 20 already cost 2e-5 of 1 / sigma over 64 channels (measured; 4.2e-5 with one run
    of 15) - the finaliser cannot return what its input does not hold."""
    return P


# ---- first-row cases for the shifted statistics pass -----------------------------------------------------------------------------------
FIRST_ROW_SIGMAS = (10.0, 100.0, 1000.0)
BELOW_GUARD_SIGMAS = (5.0, 7.5)             # |mean - K| / std below the shifted sums' recompute guard of 8
BELOW_GUARD_SHAPES = [(509, 20), (8192, 64)]
FIRST_ROW_SHAPES = [(8192, 64), (2048, 256), (509, 20)]


FIRST_ROW_MEAN = 3.0


def first_row_data(P, C, sigmas=FIRST_ROW_SIGMAS, seed=9):
    """x (P, C) float32, mean 3 and unit standard deviation per channel, except row 0: x[0, c] lies sigmas[c % len] standard deviations
    from the channel's mean (sign alternating).  Channel C - 1 is dead (every value equal), channel C - 2 has standard deviation 1e-3 and
    x[0, C - 2] off by 1.  The mean is 3 because the bar on the mean is a fraction of max |mean|: that says something only where the mean
    is not small against the spread (|mean| > std, as the data of tests/test_nn_gpu.py) - float32 sums of values x - K of size 7.5 std
    carry the mean to about 1e-6 std whatever the method.  Returns (x, the multiples per channel; 0 for the dead channel)."""
    rs = np.random.RandomState(seed + P + C)
    x = rs.standard_normal((P, C)) + FIRST_ROW_MEAN
    k = np.array([sigmas[c % len(sigmas)] * (1 if (c // len(sigmas)) % 2 == 0 else -1) for c in range(C)])
    x[:, C - 2] = FIRST_ROW_MEAN + 1e-3 * rs.standard_normal(P)
    k[C - 2] = 1000.0
    x[0] = FIRST_ROW_MEAN + k * np.where(np.arange(C) == C - 2, 1e-3, 1.0)
    x[:, C - 1] = 0.75
    k[C - 1] = 0.0
    return x.astype(np.float32), k


# ---- float64 references ---------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a, np.float64)


def bn_stats(x):
    """(mean, biased variance, 1 / sqrt(var + eps)) per channel of x (P, C): two passes in float64."""
    x = f64(x)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / np.sqrt(var + EPS)


def bn_forward(x, gamma, beta, res=None, relu=False):
    """(y, mean, var, invstd) of training-mode BatchNorm (+ residual) (+ ReLU)."""
    mean, var, invstd = bn_stats(x)
    y = f64(gamma) * ((f64(x) - mean) * invstd) + f64(beta)
    if res is not None:
        y = y + f64(res)
    if relu:
        y = np.maximum(y, 0.0)
    return y, mean, var, invstd


def running_stats(mean, var, P, run_mean0, run_var0):
    return (DECAY * f64(run_mean0) + (1 - DECAY) * mean, DECAY * f64(run_var0) + (1 - DECAY) * var * (P / max(P - 1, 1)))


def bn_backward(gy, x, gamma, mean, invstd, mask_y=None):
    """(gx, dz, ggamma, gbeta): dz = gy where mask_y > 0 (mask_y None: gy), the residual's gradient; mean / invstd as the forward saved
    them."""
    gy, x, mean, invstd = f64(gy), f64(x), f64(mean), f64(invstd)
    dz = gy if mask_y is None else np.where(np.asarray(mask_y) > 0, gy, 0.0)
    xhat = (x - mean) * invstd
    P = x.shape[0]
    gb, gg = dz.sum(0), (dz * xhat).sum(0)
    gx = f64(gamma) * invstd * (dz - gb / P - xhat * (gg / P))
    return gx, dz, gg, gb


def pair_forward(xa, gamma_a, beta_a, xb, gamma_b, beta_b):
    """relu(BN_a(xa) + BN_b(xb)) and both layers' (mean, var, invstd)."""
    r, mb, vb, sb = bn_forward(xb, gamma_b, beta_b)
    y, ma, va, sa = bn_forward(xa, gamma_a, beta_a, res=r, relu=True)
    return y, (ma, va, sa), (mb, vb, sb)


def pair_backward(gy, mask_y, xa, gamma_a, mean_a, invstd_a, xb, gamma_b, mean_b, invstd_b):
    gxa, dz, gga, gba = bn_backward(gy, xa, gamma_a, mean_a, invstd_a, mask_y)
    gxb, _, ggb, gbb = bn_backward(dz, xb, gamma_b, mean_b, invstd_b)
    return gxa, gxb, gga, gba, ggb, gbb


# ---- the same expressions in float32, in the kernels' order: the floor of the ill-conditioned cases (P <= 3, a dead channel) ------------
def _fma32(a, b, c):
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)        # a * b is exact in float64


def bn_forward_f32(x, gamma, beta, res=None, relu=False):
    """(y, mean, invstd) as k_bn_stats_partial / k_bn_stats_final / k_bn_apply compute them: float32 sums of x - x[0] in row order,
    finalised in double."""
    f = np.float32
    x = np.asarray(x, f)
    P = x.shape[0]
    K = x[0]
    a, b = np.zeros_like(K), np.zeros_like(K)
    for r in range(P):
        d = x[r] - K
        a = a + d
        b = _fma32(d, d, b)
    ms = f64(a) / P
    var = np.maximum(f64(b) / P - ms * ms, 0.0)
    mean = (f64(K) + ms).astype(f)
    invstd = (f(1) / np.sqrt(var.astype(f) + f(EPS))).astype(f)
    y = np.asarray(gamma, f) * ((x - mean) * invstd) + np.asarray(beta, f)
    if res is not None:
        y = y + np.asarray(res, f)
    if relu:
        y = np.maximum(y, f(0))
    return y, mean, invstd


def bn_backward_f32(gy, x, gamma, mean, invstd, mask_y=None):
    """(gx, ggamma, gbeta) as k_bn_bwd_partial / k_bn_bwd_final / k_bn_bwd_apply compute them, rows added in order."""
    f = np.float32
    gy, x, mean, invstd, gamma = (np.asarray(t, f) for t in (gy, x, mean, invstd, gamma))
    dz = gy if mask_y is None else np.where(np.asarray(mask_y) > 0, gy, f(0))
    xhat = (x - mean) * invstd
    P = x.shape[0]
    a, b = np.zeros(x.shape[1], f), np.zeros(x.shape[1], f)
    for r in range(P):
        a = a + dz[r]
        b = _fma32(dz[r], xhat[r], b)
    invP = f(1) / f(P)
    gx = gamma * invstd * (dz - a * invP - xhat * (b * invP))
    return gx, b, a
