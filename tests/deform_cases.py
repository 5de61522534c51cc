"""The cases of tests/test_deform_gpu.py: shapes, offset sets and the generator of the offset rows, with the tiers of csrc/deform.hip restated
as plain arithmetic.  Imports without the library or a device; tests/test_deform_cases_cpu.py holds every case against the tier it is named
for, from tests/deform_reference.list_lengths and the functions below, so a case that misses its tier fails there instead of silently
weakening the GPU comparison."""
import torch

LD = 32                                     # the padded offset row
SHAPES = [(2, 5, 7, 32), (1, 1, 1, 32), (2, 6, 5, 64)]
SETS = ['a_zero', 'b_integer', 'c_fractional', 'd_one_cell', 'e_far', 'f_few_cells']
# The tiers of the input gradient's list handling, as csrc/deform.hip has them: up to RANK_MAX entries ordered by rank, up to LIST_MAX by the
# one-wave network in LDS, longer lists by a workgroup in chunks of LONG_CHUNK, LONG_WAVES chunks per round, LONG_GRID workgroups in all.
RANK_MAX, LIST_MAX, LONG_CHUNK, LONG_WAVES, LONG_GRID = 64, 256, 128, 8, 32
ROUND = LONG_CHUNK * LONG_WAVES             # entries of one round of chunks
LONG_T = 64 * LONG_WAVES                    # threads of the long-list workgroup, one channel each
SCAN_T = 1024                               # threads of the one scan workgroup
C_MAX = 512                                 # channels the input gradient takes: two float4 accumulators per lane
# a map large enough for lists beyond one round of chunks (9 H W = 5184 entries per image) and for more long lists than workgroups
LONG_SHAPE = (1, 24, 24, 32)
LONG_SETS = ['g_targets4', 'g_targets16']
PAD_FILL = 123.0                            # what the never-read channels of a test's offset row hold

# ---- the channel tiers: the widths of res3 / res4 / res5 and the widths next to every branch on C ------------------------------------------
WIDTH_MAP = (2, 5, 7)
WIDTHS = [128, 132, 256, 260, 512]          # all three kernels
OVER_WIDTHS = [516, 1024]                   # columns and offset gradient only: the input gradient refuses C > C_MAX
WIDTH_SETS = ['b_integer', 'c_fractional', 'd_one_cell', 'f_few_cells']
WIDE_LONG = ((1, 24, 24, 512), 'g_targets4')
SLICE = 64                                  # the width of the calls a wide call is compared with, bit for bit: a tier SHAPES already pins

# ---- the scan beyond one destination per thread, C = 32 ---------------------------------------------------------------------------------------
SCAN_CASES = [((1, 32, 32, 32), ['c_fractional']),
              ((1, 25, 41, 32), ['c_fractional']),
              ((1, 33, 32, 32), ['c_fractional', 'g_targets16']),
              ((2, 40, 30, 32), ['c_fractional', 'd_one_cell', 'f_few_cells'])]
TWO_IMAGE_SHAPE = (2, 40, 30, 32)

# ---- offset row strides: version -> ld_off (no padded channel at all; the next multiple of 4; wider than LD) -----------------------------------
STRIDE_SHAPE = (2, 5, 7, 64)
STRIDES = {False: [18, 20, 40], True: [27, 28, 40]}
STRIDE_SETS = ['c_fractional', 'f_few_cells']


def offset_seed(shape):
    return 17 + sum(shape)


def used_channels(modulated):
    return 27 if modulated else 18


def make_offsets(kind, shape, modulated, seed, ld=LD):
    """The offset row (N,H,W,ld) of one set, float32 on the CPU; channels past the 18 / 27 that are read hold PAD_FILL.  The values do not
    depend on ld."""
    N, H, W, _ = shape
    g = torch.Generator().manual_seed(seed)
    off = torch.full((N, H, W, ld), PAD_FILL)
    d = torch.zeros((N, H, W, 9, 2))
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W, 1)
    ti = (torch.arange(9) // 3).float().view(1, 1, 1, 9)
    tj = (torch.arange(9) % 3).float().view(1, 1, 1, 9)
    if kind == 'b_integer':
        d = torch.randint(-2, 3, d.shape, generator=g).float()
        # positions exactly on -1 and on H / W: tap 0 of pixel (0, 0) and tap 8 of pixel (H-1, W-1) with zero offsets, and two forced ones
        d[:, 0, 0, 0] = 0
        d[:, H - 1, W - 1, 8] = 0
        d[:, H // 2, W // 2, 4, 0] = H - H // 2            # centre tap lands on row H exactly
        d[:, H // 2, W // 2, 3, 1] = -1 - (W // 2 - 1)     # tap (1, 0) lands on column -1 exactly
    elif kind == 'c_fractional':
        d = torch.randint(-2, 2, d.shape, generator=g).float() + (0.1 + 0.8 * torch.rand(d.shape, generator=g))
    elif kind == 'd_one_cell':                             # every tap of every pixel at the cell (H-1, W-1): one list of 9 H W entries
        d[..., 0] = (H - 1) - (ys - 1 + ti)
        d[..., 1] = (W - 1) - (xs - 1 + tj)
    elif kind == 'f_few_cells':
        # two taps in three aimed 0.3 / 0.6 of a cell inside one of two cells of their image, the third fractional as in (c): lists of some
        # 70 to 250 entries on eight destinations beside short ones in the same call
        d = torch.randint(-2, 2, d.shape, generator=g).float() + (0.1 + 0.8 * torch.rand(d.shape, generator=g))
        idx = torch.arange(H * W * 9).view(1, H, W, 9)
        aimed, second = (idx % 3 != 0).expand(N, H, W, 9), ((idx // 3) % 2 == 1).expand(N, H, W, 9)
        ty = torch.where(second, torch.tensor(float(max(H - 2, 0))), torch.tensor(0.0)) + 0.3
        tx = torch.where(second, torch.tensor(float(max(W - 2, 0))), torch.tensor(0.0)) + 0.6
        d[..., 0] = torch.where(aimed, ty - (ys - 1 + ti), d[..., 0])
        d[..., 1] = torch.where(aimed, tx - (xs - 1 + tj), d[..., 1])
    elif kind.startswith('g_targets'):
        # every tap of every pixel aimed 0.3 / 0.6 of a cell inside one of K cells on a grid, in turn: 4 K lists of 9 H W / K entries
        K = int(kind[len('g_targets'):])
        side = int(round(K ** 0.5))
        idx = torch.arange(H * W * 9).view(1, H, W, 9).expand(N, H, W, 9) % K
        ty = ((idx // side) * (H // side) + H // (2 * side)).float() + 0.3
        tx = ((idx % side) * (W // side) + W // (2 * side)).float() + 0.6
        d[..., 0] = ty - (ys - 1 + ti)
        d[..., 1] = tx - (xs - 1 + tj)
    elif kind == 'e_far':                                  # finite, up to 3 max(H, W), every position outside the map
        M = float(max(H, W))
        sign = torch.randint(0, 2, d.shape, generator=g).float() * 2 - 1
        d = sign * (2.5 + 0.5 * torch.rand(d.shape, generator=g)) * M
    off[..., :18] = d.reshape(N, H, W, 18)
    if modulated:
        off[..., 18:27] = 40.0 if kind == 'a_zero' else torch.randn((N, H, W, 9), generator=g)       # sigmoid(40) is 1.0f
    return off


# ---- csrc/deform.hip's branches on C and on P, as plain arithmetic ------------------------------------------------------------------------------
def group_lanes(C):
    """GL of k_deform_cols / k_deform_offset_bwd: half a wave per (pixel, tap) where C / 4 <= 32, a wave beyond."""
    return 32 if C // 4 <= 32 else 64


def channel_trips(C):
    """(the most, the fewest) trips of `for (q = gl; q < C / 4; q += GL)` over the lanes of a group; a lane with none is idle."""
    GL, C4 = group_lanes(C), C // 4
    return -(-C4 // GL), C4 // GL


def idle_lanes(C):
    return max(0, group_lanes(C) - C // 4)


def accumulator_lanes(C):
    """(lanes with the first float4 accumulator, lanes with the second) of sum_entries: `lane < C / 4`, `lane + 64 < C / 4`."""
    C4 = C // 4
    return min(64, C4), max(0, min(64, C4 - 64))


def long_live_threads(C):
    """Threads of k_deform_gather_long that keep a channel: `tid < C` of LONG_T."""
    return min(C, LONG_T)


def scan_layout(P):
    """(per, threads with a full range, threads with a partial range, idle threads) of k_deform_scan: thread t takes [t per, t per + per)
    cut at P."""
    per = -(-P // SCAN_T)
    full, rest = divmod(P, per)
    partial = 1 if rest else 0
    return per, full, partial, SCAN_T - full - partial


def scan_thread_of(dest, P):
    return dest // scan_layout(P)[0]


def slice_starts(C):
    """First channels of the SLICE-wide calls that cover C channels; the last one overlaps its neighbour where SLICE does not divide C."""
    return list(range(0, C - SLICE + 1, SLICE)) + ([C - SLICE] if C % SLICE else [])
