"""The cases that take the PointRend kernels (csrc/pointrend.hip, csrc/point_common.h) past five rows, one
ballot, one lane trip and one grid pass, and the kernels' thread maps restated as plain arithmetic.  Imports without the library or a
device: tests/test_pointrend_edge_cases_cpu.py holds every case to the path it is named for, tests/test_pointrend_edges_gpu.py compares
kernel and reference (tests/pointrend_reference.py) on them.  The builders are cached: a case and its reference are computed once.

A helper of the tests, not a test and not part of the product."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointrend_reference as pr            # noqa: E402

F32, F64 = np.float32, np.float64
SCALE = 0.25                    # the stride-4 level

# ---- the thread maps ------------------------------------------------------------------------------------------------------------------------
NT, WAVE = 256, 64              # threads of a workgroup, lanes of a wave
PB_H, PB_W = 2, 4               # cells of the patch a wave of k_point_features_bwd owns
PB_WAVES = NT // WAVE           # patches per workgroup
GRID_CAP = 65535                # workgroups of the elementwise kernels (ew_blocks)
LOSS_BLOCKS = 1024              # workgroups of the loss kernels (grid_for)
LDS_BYTES = 64 * 1024           # dynamic LDS k_point_features_bwd may ask for
PT_MAX_CAND = 4096              # candidates the LDS sort of k_point_train_coords holds
SD_MAX_S = 56                   # the largest grid k_point_subdivide upsamples into LDS
SD_T = 1024                     # its threads


def cdiv(a, b):
    return -(-a // b)


def tiles(H, W):
    return cdiv(W, PB_W), cdiv(H, PB_H)


def n_patches(N, H, W):
    tx, ty = tiles(H, W)
    return N * tx * ty


def patch_of(img, y, x, H, W):
    """The patch (= wave) that owns cell (y, x) of image img."""
    tx, ty = tiles(H, W)
    return (img * ty + y // PB_H) * tx + x // PB_W


def bwd_workgroups(N, H, W):
    return cdiv(n_patches(N, H, W), PB_WAVES)


def bwd_idle_waves(N, H, W):
    """Waves of the last workgroup that leave at `patch >= n_patches`."""
    return bwd_workgroups(N, H, W) * PB_WAVES - n_patches(N, H, W)


def bwd_lds_bytes(C):
    return PB_WAVES * PB_H * PB_W * C * 4


def lane_trips(C):
    """Trips of the `q += 64` loops over the float4s of C channels."""
    return cdiv(C // 4, WAVE)


def ballot_trips(n):
    """Trips of a `+= 64` ballot loop over n rows or points."""
    return cdiv(n, WAVE)


def fwd_grid(n_points):
    """Workgroups of k_point_features_fwd: a wave per point, capped."""
    return max(1, min(cdiv(n_points * WAVE, NT), GRID_CAP))


def fwd_passes(n_points):
    return cdiv(n_points, fwd_grid(n_points) * PB_WAVES)


def loss_grid(n):
    return max(1, min(cdiv(n, NT), LOSS_BLOCKS))


def loss_trips(n):
    return cdiv(n, loss_grid(n) * NT)


def sort_size(n_cand):
    n2 = 2
    while n2 < n_cand:
        n2 <<= 1
    return n2


def ceil4(n):
    return cdiv(n, 4) * 4


# ---- where the taps of a feature case land -----------------------------------------------------------------------------------------------------
def tap_table(c, dt=F32):
    """Every tap of the fine sampling that lands inside the map, in the kernel's (row, point, tap) order: dict of flat int arrays row,
    point, tap, img, y, x, patch."""
    N, H, W = c['fmap'].shape[:3]
    rows, P = c['coords'].shape[:2]
    X, Y = pr.frame(c['rois'], c['coords'], dt)
    sc = dt(np.float32(SCALE))
    x0, y0, _ = pr.taps(X * sc, Y * sc, W, H, dt)
    img = c['rois'][:, 0].astype(np.int64)
    k = np.arange(4)
    x = x0[..., None] + (k & 1)
    y = y0[..., None] + (k >> 1)
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H) & ((img >= 0) & (img < N))[:, None, None]
    r, p, t = np.nonzero(ok)
    out = dict(row=r, point=p, tap=t, img=img[r], y=y[ok], x=x[ok])
    out['patch'] = np.array([patch_of(i, yy, xx, H, W) for i, yy, xx in zip(out['img'], out['y'], out['x'])], np.int64)
    return out


def taps_per_cell(c, dt=F32):
    N, H, W = c['fmap'].shape[:3]
    t = tap_table(c, dt)
    n = np.zeros((N, H, W), np.int64)
    np.add.at(n, (t['img'], t['y'], t['x']), 1)
    return n


# ---- point_features_bwd / point_features_fwd ----------------------------------------------------------------------------------------------------
def _boxes(rows):
    return np.zeros((len(rows), 5), np.float32) + np.asarray(rows, np.float32)


def _case(N, H, W, C, P, rows, seed, n_fg=3, S0=6, cin_p=None, **kw):
    return pr.general_feature_case(N, H, W, C, P, rows, n_fg, S0, pr.pad32(C + n_fg) if cin_p is None else cin_p, seed, **kw)


def _ballot_rois(rows, H, W, seed):
    """Rows below 64 stay in the left half of the map; the rows from 64 on cover the whole map, so they share patches with the first
    block of rows and are the first rows on patches of the right half."""
    rs = np.random.RandomState(seed)
    fh, fw = 4.0 * H, 4.0 * W
    rois = np.zeros((rows, 5), np.float32)
    rois[:, 0] = np.arange(rows) % 2
    rois[:, 1], rois[:, 2] = rs.uniform(-0.1, 0.2, rows) * fw, rs.uniform(-0.1, 0.5, rows) * fh
    rois[:, 3], rois[:, 4] = rois[:, 1] + rs.uniform(0.05, 0.25, rows) * fw, rois[:, 2] + rs.uniform(0.1, 0.5, rows) * fh
    rois[64:, 1:] = (0.0, 0.0, fw, fh)
    return rois


CENTRE_UV = (0.0, 0.25, 0.5, 0.75)          # of the box (2, 2, 18, 18): X = 2 + 16 u = 4 (i + 0.5), the centres of cells 0 .. 3
NAN_PAYLOAD = 0x7fc12345                    # the prior of an image no tap lands on


def _outside_rois(N, H, W):
    fh, fw = 4.0 * H, 4.0 * W
    return _boxes([[0, -40.0, 4.0, -8.0, 20.0],                  # left of the map
                   [1, fw + 8.0, 4.0, fw + 40.0, 20.0],          # right of it
                   [0, 4.0, -40.0, 30.0, -8.0],                  # above
                   [1, 4.0, fh + 8.0, 30.0, fh + 40.0],          # below
                   [-1, 4.0, 4.0, 30.0, 30.0],                   # image index -1
                   [N, 4.0, 4.0, 30.0, 30.0]])                   # image index N


@functools.lru_cache(maxsize=None)
def feature_cases():
    """name -> case (the dict of pr.general_feature_case) for the backward and forward feature kernels."""
    H, W = 9, 13
    fh, fw = 4.0 * H, 4.0 * W
    out = {}
    # 1. the row ballot takes a second (and third) trip
    for rows in (65, 130):
        out['ballot rows %d' % rows] = _case(2, H, W, 32, 7, rows, 10 + rows, rois=_ballot_rois(rows, H, W, rows))
    # 2. hundreds of taps on one cell: the (row, point, tap) order decides the bits; the point ballot takes a second trip
    small = np.tile(np.array([[0, 17.0, 13.0, 23.0, 19.0]], np.float32), (130, 1))
    out['ordered sum'] = _case(2, H, W, 8, 65, 130, 21, rois=small)
    # 3. channels: one float4, a second lane trip, the LDS limit; ld == C and ld > C
    for C, ld in ((4, 32), (260, 260), (512, 544)):
        out['channels %d ld %d' % (C, ld)] = _case(2, H, W, C, 7, 5, 30 + C, ld=ld)
    out['channels 516'] = _case(2, H, W, 516, 7, 5, 33)
    # 4. patch geometry
    out['map 1x1'] = _case(1, 1, 1, 8, 7, 5, 41, rois=_boxes([[0, -3, -2, 6, 5], [0, 0, 0, 4, 4], [0, 1, 1, 3, 3], [0, 2, -4, 9, 3], [0, -1, 0, 2, 8]]))
    out['map 2x4'] = _case(1, 2, 4, 8, 7, 5, 42)
    out['map 5x5'] = _case(1, 5, 5, 8, 7, 5, 43, rois=_boxes([[0, -2, -2, 22, 22], [0, 0, 0, 20, 20], [0, 13, 13, 24, 24], [0, 1, 12, 19, 21],
                                                            [0, 14, 0, 21, 9]]))
    c = _case(3, H, W, 8, 7, 6, 44)
    c['rois'][:, 0] = (0, 2, 2, 0, 2, 0)
    c['g_map'][1] = np.full((H, W, 8), NAN_PAYLOAD, np.uint32).view(np.float32)
    out['image 1 untouched'] = c
    # 5. boxes
    c = _case(2, H, W, 8, 7, 5, 51, rois=_boxes([[0, 0.7 * fw, 0.8 * fh, 0.2 * fw, 0.1 * fh],           # inverted
                                               [1, 0.4 * fw, 0.3 * fh, 0.4 * fw, 0.3 * fh],           # zero extent
                                               [0, 2.0, 2.0, 18.0, 18.0],                             # its points are cell centres
                                               [1, 0.1 * fw, 0.2 * fh, 0.6 * fw, 0.9 * fh],           # ordinary
                                               [0, 0.5 * fw, 0.5 * fh, 0.5 * fw, 0.9 * fh]]))         # zero width only
    uv = np.array([(u, v) for v in CENTRE_UV for u in CENTRE_UV], np.float32)
    c['coords'][2] = uv[:7]
    out['boxes'] = c
    out['huge box'] = _case(2, H, W, 8, 7, 3, 52, rois=_boxes([[0, -1e9, -1e9, 1e9, 1e9], [1, 1e9, -1e9, -1e9, 1e9], [0, 4.0, 4.0, 40.0, 30.0]]))
    out['outside'] = _case(2, H, W, 8, 7, 6, 53, rois=_outside_rois(2, H, W))
    # 7. the coarse part: where the logical channels end inside a float4, an input they fill exactly, zeros behind; S0 = 1 and 7
    for n_fg, S0 in ((1, 1), (2, 7), (4, 1), (5, 7), (80, 1)):
        need = ceil4(32 + n_fg)
        for cin_p in ((need,) if n_fg == 4 else (need + 8,)):
            out['coarse n_fg %d S0 %d cin_p %d' % (n_fg, S0, cin_p)] = _case(2, H, W, 32, 7, 5, 70 + n_fg, n_fg=n_fg, S0=S0, cin_p=cin_p)
    return out


BWD_CASES = ('ballot rows 65', 'ballot rows 130', 'ordered sum', 'channels 4 ld 32', 'channels 260 ld 260', 'channels 512 ld 544', 'map 1x1',
             'map 2x4', 'map 5x5', 'image 1 untouched', 'boxes', 'huge box', 'outside')
BWD_REFUSED = 'channels 516'
FWD_CASES = ('channels 4 ld 32', 'channels 260 ld 260', 'channels 512 ld 544', 'channels 516', 'boxes', 'huge box', 'outside', 'image 1 untouched',
             'coarse n_fg 1 S0 1 cin_p 44', 'coarse n_fg 2 S0 7 cin_p 44', 'coarse n_fg 4 S0 1 cin_p 36', 'coarse n_fg 5 S0 7 cin_p 48',
             'coarse n_fg 80 S0 1 cin_p 120')


@functools.lru_cache(maxsize=None)
def second_pass_case():
    """rows * P > 4 * 65535: the grid-stride loop of k_point_features_fwd takes a second trip."""
    return pr.general_feature_case(2, 9, 13, 4, 196, 1400, 1, 2, 32, 80)


# ---- point_concat_* -------------------------------------------------------------------------------------------------------------------------
CONCAT_CH = (4, 256)
CONCAT_COARSE = ((0, 1), (256, 3), (256, 4), (260, 5), (256, 80))
CONCAT_POINTS = (1, 1000)


def concat_shapes(Ch, c0, n_coarse):
    """[(ld0, cin_p)]: the smallest legal and a larger value of each."""
    ld0, cin_p = ceil4(c0 + n_coarse), ceil4(Ch + n_coarse)
    return [(ld0, cin_p), (ld0 + 32, cin_p), (ld0, cin_p + 24), (ld0 + 32, cin_p + 24)]


def concat_case(Ch, c0, n_coarse, ld0, cin_p, n_points):
    rs = np.random.RandomState(Ch + c0 + n_coarse + ld0 + cin_p + n_points)
    h = rs.standard_normal((n_points, Ch)).astype(F32)
    x0 = rs.standard_normal((n_points, ld0)).astype(F32)
    x0[x0 == 0] = 1.0
    return dict(h=h, x0=x0, g_in=rs.standard_normal((n_points, cin_p)).astype(F32))


# ---- point_train_coords ---------------------------------------------------------------------------------------------------------------------
COORD_CANDS = (1, 2, 256, 257, 4096)
COORD_P = (1, 196)
COORD_S0 = (1, 28)
COORD_N_FG = 3


def _keys(rs, rows, n):
    return rs.randint(0, 2 ** 32, (rows, n), dtype=np.uint64).astype(np.uint32).view(np.int32)


def coords_case(n_cand, P, S0, full):
    """Three rows (the first class, the last class, background); n_imp = 0, or min(P, n_cand) when ``full``."""
    n_imp = min(P, n_cand) if full else 0
    rs = np.random.RandomState(n_cand * 7 + P + S0 + full)
    Cp = pr.pad32(COORD_N_FG)
    return dict(keys=_keys(rs, 3, 2 * n_cand + 2 * (P - n_imp)), coarse=(rs.standard_normal((3, S0, S0, Cp)) * 2).astype(F32),
                label=np.array([1, COORD_N_FG, 0], np.int32), n_fg=COORD_N_FG, P=P, n_cand=n_cand, n_imp=n_imp)


@functools.lru_cache(maxsize=None)
def special_coords_case():
    """P = n_cand = n_imp = 256 on an 8 x 8 grid, so the whole ranked list is the output.  Row 0: the selected channel is constant down
    every column and holds, column by column, 0, -0.0, -0.0, a denormal, a negative denormal, +inf, -inf, NaN - candidates between two
    columns mix them (inf next to -inf gives NaN).  Row 1: every key has all bits set - every coordinate is 1 - 2^-24.  Row 2: ordinary."""
    rs = np.random.RandomState(5)
    n = 256
    Cp = pr.pad32(COORD_N_FG)
    coarse = (rs.standard_normal((3, 8, 8, Cp)) * 2).astype(F32)
    tiny = np.float32(2.0 ** -140)
    coarse[0, :, :, 1] = np.array([0.0, -0.0, -0.0, tiny, -3 * tiny, np.inf, -np.inf, np.nan], F32)[None, :]
    keys = _keys(rs, 3, 2 * n)
    keys[1] = -1
    return dict(keys=keys, coarse=coarse, label=np.array([2, 1, 3], np.int32), n_fg=COORD_N_FG, P=n, n_cand=n, n_imp=n)


# ---- point_subdivide / point_scatter --------------------------------------------------------------------------------------------------------
SUB_S = (1, 3, 17, 56)
SUB_LD, SUB_N_CH = 8, 3
SUB_LABEL = np.array([1, 2, 0, -1, SUB_N_CH], np.int32)         # the last two select no class: channel 0
SPECIALS = (np.inf, -np.inf, np.nan)


@functools.lru_cache(maxsize=None)
def subdivide_case(S):
    """Five detections on (S,S,8) grids, every channel non-zero: 0 random, 1 all zero in its channel (the tie rule alone selects), 2 with
    +-inf and NaN sprinkled over its channel, 3 and 4 with labels -1 and n_channels (a padding channel that holds other data)."""
    rs = np.random.RandomState(S)
    grid = (rs.standard_normal((5, S, S, SUB_LD)) * 2).astype(F32)
    grid[grid == 0] = 1.0
    grid[1, :, :, 2] = 0.0
    flat = grid[2, :, :, 0].reshape(-1)
    pos = rs.permutation(S * S)[:max(1, min(S * S // 3, 12))]
    flat[pos] = np.array([SPECIALS[i % 3] for i in range(len(pos))], F32)
    grid[2, :, :, 0] = flat.reshape(S, S)
    return dict(grid=grid, label=SUB_LABEL.copy(), n_channels=SUB_N_CH)


def chosen_channel(label, n_channels):
    label = np.asarray(label)
    return np.where((label >= 0) & (label < n_channels), label, 0)


def chosen_grids(c):
    return c['grid'][np.arange(len(c['label'])), :, :, chosen_channel(c['label'], c['n_channels'])]


# ---- point_target ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def target_case(H, W):
    """N = 3, G = 1, n_sample = 3, rows = 2, P = 196 on an H x W image whose masks are all ones: row 0 of every image covers the image,
    row 1 of image 0 lies wholly outside it (a live row, every target zero), row 1 of image 2 is background."""
    rs = np.random.RandomState(H * 10 + W)
    N, rows, S, P = 3, 2, 3, 196
    rois = np.zeros((N * rows, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), rows)
    rois[:, 1:] = (-0.5, -0.5, W + 0.5, H + 0.5)
    rois[1, 1:] = (W + 2.0, H + 2.0, W + 9.0, H + 6.0)
    masks = np.full((N, 1, H, W), 255, np.uint8)
    masks[1, 0, 0, ::2] = 0
    return dict(masks=masks, n_gt=np.ones((N,), np.int32), rois=rois, gt_assign=np.zeros((N * S,), np.int32),
                label=np.array([1, 2, 1, 1, 3, 0], np.int32), n_pos=np.array([2, 2, 2], np.int32), n_sample=S, rows=rows,
                coords=rs.rand(N * rows, P, 2).astype(F32))


# ---- point_bce ------------------------------------------------------------------------------------------------------------------------------
def bce_case(rows, P, ld, n_fg, seed=0):
    """Random logits and targets; row 1 is not live, row 2 is background, row 3's label is n_fg + 1 (past the last class; a real column
    of pred where ld > n_fg)."""
    rs = np.random.RandomState(seed + rows + P)
    pred = (rs.standard_normal((rows, 1, P, ld)) * 3).astype(F32)
    tgt = rs.rand(rows, P).astype(F32)
    tgt[rs.rand(rows, P) < 0.3] = 0.0
    tgt[rs.rand(rows, P) < 0.3] = 1.0
    label = rs.randint(1, n_fg + 1, rows).astype(np.int32)
    tgt[1] = -1.0
    label[2] = 0
    label[3] = n_fg + 1
    label[-1] = n_fg
    return dict(pred=pred, target=tgt, label=label, n_fg=n_fg)


BCE_CASES = {'strided': (1400, 196, 4, 4), 'one point': (9, 1, 8, 3)}
