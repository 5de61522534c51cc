// Mask-IoU counts of the instance-segmentation evaluator on gfx950 (chainer_maskrcnn/evaluations.py): exact integer
// intersections and areas between every mask of a and every mask of b at full image resolution.  Replaces ChainerCV's
// host mask_iou (evaluations/mask_iou.py: bitwise_and(...).sum() / bitwise_or(...).sum() per pair, in NumPy).
//   zero : the outputs (inter, area_a, area_b) are zeroed - the two passes below accumulate into them with integer atomics,
//          so the result does not depend on the decomposition.
//   pack : one byte per pixel -> one bit per pixel, 64 consecutive pixels per 64-bit word, tail zero-padded; the areas.
//          HBM-bound: each wave reads aligned 1 KiB windows of a row with one 16-byte load per lane, kUnroll windows at once.
//   popc : inter[i][j] = sum_w popc(a_w & b_w) over 16 x 16 mask tiles and a split of the word range; labelled calls skip
//          cross-label pairs (and tiles without a same-label pair) before any word is read.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int kPackBlock = 256;                  // 4 waves; a window = 1 KiB of a row = 16 words
constexpr int kTile = 16;                        // popc: 16 x 16 mask pairs per workgroup, one pair per thread
constexpr int kChunk = 64;                       // popc: words per LDS stage
constexpr int kTargetBlocks = 2048;              // enough workgroups to fill 256 CUs several times over
constexpr int kUnroll = 4;                       // pack: windows per wave and step (loads in flight)

// 16 bits = (byte != 0) for the 16 bytes of v, byte k -> bit k.
__device__ __forceinline__ unsigned nonzero_bits4(unsigned v) {
    const unsigned t = ((((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u) >> 7;     // 0/1 per byte
    return ((t * 0x01020408u) >> 24) & 0xFu;                                             // byte i -> bit i
}

// Bits of the 16-byte chunk that starts at row position pos (pos = -s mod 16, so row + pos is 16-byte aligned); bytes
// outside [0, HW) read as 0.  A chunk that overlaps the row lies in the same aligned 16-byte granule as a byte of the row,
// so the one load never leaves the row's pages; a chunk entirely outside the row is not loaded.
__device__ __forceinline__ unsigned chunk_bits(const unsigned char *__restrict__ row, long long pos, long long HW) {
    if (pos >= HW || pos + 16 <= 0) return 0u;
    const uint4 v = *reinterpret_cast<const uint4 *>(row + pos);
    unsigned bits = nonzero_bits4(v.x) | (nonzero_bits4(v.y) << 4) | (nonzero_bits4(v.z) << 8) | (nonzero_bits4(v.w) << 12);
    const int lo = pos < 0 ? (int)-pos : 0;
    const int hi = HW - pos < 16 ? (int)(HW - pos) : 16;
    return bits & ((0xFFFFu >> (16 - hi)) & (0xFFFFu << lo));
}

__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void k_mask_iou_zero(int32_t *__restrict__ area_a, int Da, int32_t *__restrict__ area_b, int Db,
                                                      int32_t *__restrict__ inter, long long n_inter) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_inter + Da + Db; i += stride) {
        if (i < n_inter) inter[i] = 0;
        else if (i < n_inter + Da) area_a[i - n_inter] = 0;
        else area_b[i - n_inter - Da] = 0;
    }
}

// grid (x: windows, y: masks of a then b).  Window k of a row covers the aligned bytes [A0 + 1024 k, A0 + 1024 k + 1024),
// A0 = row start rounded down to 16 bytes, s = row start - A0.  Lane L turns its 16 bytes into 16 bits; the four lanes of
// group j OR theirs into G_j (window offsets [64 j, 64 j + 64)).  Word 16 k + j covers row positions [64 (16 k + j), +64) =
// window offsets [64 j + s, +64): (G_j >> s) | (low s bits of the next group's first chunk << (64 - s)); s < 16, so one
// chunk of the next group is enough (for j = 15 lane 60 loads the first chunk of the next window itself).
__global__ __launch_bounds__(kPackBlock) void k_mask_pack(const unsigned char *__restrict__ a, int Da, const unsigned char *__restrict__ b,
                                                          int Db, long long HW, long long NW, u64 *__restrict__ words,
                                                          int32_t *__restrict__ area_a, int32_t *__restrict__ area_b) {
    __shared__ unsigned s_cnt[kPackBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const long long nwin = (NW + 15) / 16;
    for (long long d = blockIdx.y; d < (long long)Da + Db; d += gridDim.y) {
        const unsigned char *row = d < Da ? a + d * HW : b + (d - Da) * HW;
        u64 *out = words + d * NW;
        const int s = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        unsigned cnt = 0;
        // kUnroll consecutive windows per wave and step: all their loads are issued before the first is used
        for (long long win0 = ((long long)blockIdx.x * (kPackBlock / kWave) + wv) * kUnroll; win0 < nwin;
             win0 += (long long)gridDim.x * (kPackBlock / kWave) * kUnroll) {
            unsigned bits[kUnroll], next[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long pos = (win0 + u) * 1024 + lane * 16 - s;          // past the row (win0 + u >= nwin): not loaded
                bits[u] = chunk_bits(row, pos, HW);
                next[u] = lane == kWave - 4 ? chunk_bits(row, pos + 64, HW) : 0u;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                u64 g = (u64)bits[u] << (16 * (lane & 3));
                g |= shfl_xor64(g, 1);
                g |= shfl_xor64(g, 2);
                unsigned nb = __shfl(bits[u], (lane + 4) & (kWave - 1));
                if (lane == kWave - 4) nb = next[u];
                const long long w = (win0 + u) * 16 + (lane >> 2);
                if ((lane & 3) == 0 && w < NW) {
                    const u64 word = s ? (g >> s) | ((u64)nb << (64 - s)) : g;
                    out[w] = word;
                    cnt += (unsigned)__popcll(word);
                }
            }
        }
        for (int m = kWave / 2; m > 0; m >>= 1) cnt += __shfl_xor(cnt, m);
        if (lane == 0) s_cnt[wv] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned t = 0;
            for (int i = 0; i < kPackBlock / kWave; ++i) t += s_cnt[i];
            if (t) atomicAdd(d < Da ? area_a + d : area_b + (d - Da), (int32_t)t);
        }
        __syncthreads();
    }
}

// grid (x: 16 x 16 tiles of (a, b) pairs, y: word ranges of wps words).  One pair per thread; both tiles' words are staged
// through LDS transposed ([word][mask], row padded to 17) so that a wave's 16 b-masks read one contiguous 128-byte run.
__global__ __launch_bounds__(kTile * kTile) void k_mask_and_popc(const u64 *__restrict__ wa, int Da, const u64 *__restrict__ wb, int Db,
                                                                 long long NW, long long wps, int ntj, const int32_t *__restrict__ la,
                                                                 const int32_t *__restrict__ lb, int32_t *__restrict__ inter) {
    __shared__ u64 sA[kChunk][kTile + 1], sB[kChunk][kTile + 1];
    __shared__ int liveA[kTile], liveB[kTile];
    const int t = threadIdx.x, ti = t / kTile, tj = t % kTile;
    const long long i0 = (long long)(blockIdx.x / ntj) * kTile, j0 = (long long)(blockIdx.x % ntj) * kTile;
    const long long i = i0 + ti, j = j0 + tj;
    if (t < kTile) { liveA[t] = 0; liveB[t] = 0; }
    __syncthreads();
    const bool live = i < Da && j < Db && (la == nullptr || la[i] == lb[j]);
    if (live) { liveA[ti] = 1; liveB[tj] = 1; }
    if (!__syncthreads_or(live)) return;                              // no same-label pair in the tile: no word work
    const long long w_begin = (long long)blockIdx.y * wps, w_end = min(NW, w_begin + wps);
    unsigned acc = 0;
    for (long long w0 = w_begin; w0 < w_end; w0 += kChunk) {
        for (int e = t; e < kTile * kChunk; e += kTile * kTile) {
            const int r = e / kChunk, k = e % kChunk;
            const long long w = w0 + k;
            if (liveA[r]) sA[k][r] = w < w_end ? wa[(i0 + r) * NW + w] : 0ull;
            if (liveB[r]) sB[k][r] = w < w_end ? wb[(j0 + r) * NW + w] : 0ull;
        }
        __syncthreads();
        if (live) {
#pragma unroll 8
            for (int k = 0; k < kChunk; ++k) acc += (unsigned)__popcll(sA[k][ti] & sB[k][tj]);
        }
        __syncthreads();
    }
    if (live && acc) atomicAdd(inter + i * Db + j, (int32_t)acc);
}

long long words_per_mask(long long HW) { return (HW + 63) / 64; }

// ---- Boundary IoU (Cheng et al., CVPR 2021): the boundary band B = M & ~erode_d(M) of every mask, and the counts of the bands ------------
//   rows  : the byte masks packed ROW-ALIGNED, (mask, y) -> ceil(W / 64) words, tail bits zero (they double as the background right of the
//           image); the mask areas.  Same window arithmetic as k_mask_pack, a window being 1 KiB of one image row.
//   band  : per (mask, band of kBandRows rows, kBandCols word columns) the d-fold 3 x 3 erosion as two separable passes, a horizontal one
//           on a 192-bit (left, own, right) window in registers and a vertical one in LDS over the band and its d-row halos, both as
//           O(log d) shift-AND (row-offset AND) doubling steps; then B, and the band areas by one integer atomic per workgroup.
//   The AND-popcount kernel above then runs twice, on the mask words and on the band words (any layout both sides share).
constexpr int kMaxDilation = 63;                 // a horizontal shift stays within the neighbouring word
constexpr int kBandRows = 64;                    // rows of one band tile (ops.BOUNDARY_BAND_ROWS)
constexpr int kBandCols = 8;                     // word columns of one band tile
constexpr int kBandExt = kBandRows + 2 * kMaxDilation;
constexpr int kBandBlock = 256;

// grid (x: window slices of a mask's H * nwin row windows, y: masks of a then b); see k_mask_pack for the window arithmetic
__global__ __launch_bounds__(kPackBlock) void k_mask_pack_rows(const unsigned char *__restrict__ a, int Da, const unsigned char *__restrict__ b,
                                                               int Db, int H, int W, int NWr, u64 *__restrict__ words,
                                                               int32_t *__restrict__ area_a, int32_t *__restrict__ area_b) {
    __shared__ unsigned s_cnt[kPackBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int nwin = (NWr + 15) / 16;
    const long long nitem = (long long)H * nwin, HW = (long long)H * W;
    for (long long d = blockIdx.y; d < (long long)Da + Db; d += gridDim.y) {
        const unsigned char *mask = d < Da ? a + d * HW : b + (d - Da) * HW;
        u64 *out = words + d * H * NWr;
        unsigned cnt = 0;
        for (long long it0 = ((long long)blockIdx.x * (kPackBlock / kWave) + wv) * kUnroll; it0 < nitem;
             it0 += (long long)gridDim.x * (kPackBlock / kWave) * kUnroll) {
            unsigned bits[kUnroll], next[kUnroll];
            int sh[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long it = it0 + u;
                bits[u] = next[u] = 0u;
                sh[u] = 0;
                if (it < nitem) {
                    const unsigned char *row = mask + (it / nwin) * W;
                    sh[u] = (int)(reinterpret_cast<uintptr_t>(row) & 15);
                    const long long pos = (it % nwin) * 1024 + lane * 16 - sh[u];
                    bits[u] = chunk_bits(row, pos, W);
                    if (lane == kWave - 4) next[u] = chunk_bits(row, pos + 64, W);
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const long long it = it0 + u;
                u64 g = (u64)bits[u] << (16 * (lane & 3));
                g |= shfl_xor64(g, 1);
                g |= shfl_xor64(g, 2);
                unsigned nb = __shfl(bits[u], (lane + 4) & (kWave - 1));
                if (lane == kWave - 4) nb = next[u];
                const int w = (int)(it % nwin) * 16 + (lane >> 2);
                if ((lane & 3) == 0 && it < nitem && w < NWr) {
                    const int s = sh[u];
                    const u64 word = s ? (g >> s) | ((u64)nb << (64 - s)) : g;
                    out[(it / nwin) * NWr + w] = word;
                    cnt += (unsigned)__popcll(word);
                }
            }
        }
        if (area_a != nullptr || area_b != nullptr) {                 // uniform: the words entry asks for no areas
            for (int m = kWave / 2; m > 0; m >>= 1) cnt += __shfl_xor(cnt, m);
            if (lane == 0) s_cnt[wv] = cnt;
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned t = 0;
                for (int i = 0; i < kPackBlock / kWave; ++i) t += s_cnt[i];
                if (t) atomicAdd(d < Da ? area_a + d : area_b + (d - Da), (int32_t)t);
            }
            __syncthreads();
        }
    }
}

struct U192 { u64 lo, mid, hi; };                // bit k of lo, mid, hi = position k, 64 + k, 128 + k

// v >> r over the 192 bits, zeros coming in at the top; 1 <= r <= 63
__device__ __forceinline__ U192 shr192(U192 v, int r) {
    return {(v.lo >> r) | (v.mid << (64 - r)), (v.mid >> r) | (v.hi << (64 - r)), v.hi >> r};
}

// The own word of the horizontal erosion of radius d (1..63): bit j = AND of positions 64 + j - d .. 64 + j + d of (left, own, right).
// A_r[x] = AND of r positions from x on; A_2r = A_r & (A_r >> r), A_n = A_p & (A_p >> (n - p)) for n = 2 d + 1 and the largest power of
// two p <= n (n is odd, so 1 <= n - p < p <= 64).  The zeros that the shifts bring in reach A_n[x] only for x + n > 192; the bits read are
// x in [64 - d, 128 - d).
__device__ __forceinline__ u64 erode_row(u64 left, u64 own, u64 right, int d) {
    const int n = 2 * d + 1;
    U192 v = {left, own, right};
    int r = 1;
    for (; 2 * r <= n; r *= 2) {
        const U192 s = shr192(v, r);
        v = {v.lo & s.lo, v.mid & s.mid, v.hi & s.hi};
    }
    const U192 s = shr192(v, n - r);
    v = {v.lo & s.lo, v.mid & s.mid, v.hi & s.hi};
    return (v.lo >> (64 - d)) | (v.mid << d);
}

__device__ __forceinline__ u64 row_word(const u64 *__restrict__ m, int H, int NWr, int y, int w) {
    return (y >= 0 && y < H && w >= 0 && w < NWr) ? m[(long long)y * NWr + w] : 0ull;        // outside the image: background
}

// grid (x: band tiles = row bands x column groups, y: masks).  LDS row e of the tile is image row y0 - d + e, e < ne = rows + 2 d.
__global__ __launch_bounds__(kBandBlock) void k_mask_boundary(const u64 *__restrict__ words, long long nmask, int Da, int H, int NWr, int d,
                                                              int ncol, u64 *__restrict__ bwords, int32_t *__restrict__ barea_a,
                                                              int32_t *__restrict__ barea_b) {
    __shared__ u64 sE[2][kBandExt][kBandCols];
    __shared__ unsigned s_cnt[kBandBlock / kWave];
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int y0 = (int)(blockIdx.x / ncol) * kBandRows, c0 = (int)(blockIdx.x % ncol) * kBandCols;
    const int rows = min(kBandRows, H - y0), cols = min(kBandCols, NWr - c0), ne = rows + 2 * d, n = 2 * d + 1;
    for (long long k = blockIdx.y; k < nmask; k += gridDim.y) {
        const u64 *m = words + k * H * NWr;
        for (int e = t; e < ne * kBandCols; e += kBandBlock) {
            const int r = e / kBandCols, c = e % kBandCols, y = y0 - d + r, w = c0 + c;
            sE[0][r][c] = c < cols ? erode_row(row_word(m, H, NWr, y, w - 1), row_word(m, H, NWr, y, w), row_word(m, H, NWr, y, w + 1), d) : 0ull;
        }
        __syncthreads();
        // vertical: A_r[e] = AND of rows e .. e + r - 1; rows past the tile stand in as all ones (the rows read below never need them)
        int cur = 0, r = 1;
        for (;;) {
            const int step = 2 * r <= n ? r : n - r;
            for (int e = t; e < ne * kBandCols; e += kBandBlock) {
                const int row = e / kBandCols, c = e % kBandCols;
                sE[cur ^ 1][row][c] = sE[cur][row][c] & (row + step < ne ? sE[cur][row + step][c] : ~0ull);
            }
            __syncthreads();
            cur ^= 1;
            if (2 * r > n) break;
            r *= 2;
        }
        unsigned cnt = 0;
        u64 *out = bwords + k * H * NWr;
        for (int e = t; e < rows * kBandCols; e += kBandBlock) {
            const int row = e / kBandCols, c = e % kBandCols;
            if (c < cols) {
                const long long at = (long long)(y0 + row) * NWr + c0 + c;
                const u64 bw = m[at] & ~sE[cur][row][c];
                out[at] = bw;
                cnt += (unsigned)__popcll(bw);
            }
        }
        if (barea_a != nullptr || barea_b != nullptr) {               // uniform: the words entry asks for no areas
            for (int s = kWave / 2; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
            if (lane == 0) s_cnt[wv] = cnt;
            __syncthreads();
            if (t == 0) {
                unsigned sum = 0;
                for (int i = 0; i < kBandBlock / kWave; ++i) sum += s_cnt[i];
                if (sum) atomicAdd(k < Da ? barea_a + k : barea_b + (k - Da), (int32_t)sum);
            }
        }
        __syncthreads();
    }
}

long long words_per_row(int W) { return ((long long)W + 63) / 64; }

// rows + band for nmask = Da + Db masks: mwords and bwords (nmask, H, NWr) each; area / barea NULL = not wanted
int launch_boundary_stage(const unsigned char *a, int Da, const unsigned char *b, int Db, int H, int W, int dilation, u64 *mwords, u64 *bwords,
                          int32_t *area_a, int32_t *area_b, int32_t *barea_a, int32_t *barea_b, hipStream_t st) {
    const long long nmask = (long long)Da + Db;
    const int NWr = (int)words_per_row(W), nwin = (NWr + 15) / 16;
    const long long nitem = (long long)H * nwin;
    const long long gx = std::max(1LL, std::min((nitem + 4 * kUnroll - 1) / (4 * kUnroll), (kTargetBlocks + nmask - 1) / nmask));
    const unsigned gy = (unsigned)std::min(nmask, 65535LL);
    hipLaunchKernelGGL(k_mask_pack_rows, dim3((unsigned)gx, gy), dim3(kPackBlock), 0, st, a, Da, b, Db, H, W, NWr, mwords, area_a, area_b);
    MRCNN_LAUNCH_CHECK();
    const int ncol = (NWr + kBandCols - 1) / kBandCols;
    const long long ntile = (long long)((H + kBandRows - 1) / kBandRows) * ncol;
    hipLaunchKernelGGL(k_mask_boundary, dim3((unsigned)ntile, gy), dim3(kBandBlock), 0, st, mwords, nmask, Da, H, NWr, dilation, ncol, bwords,
                       barea_a, barea_b);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

// the size checks the two boundary entries share; 0 = fine
int check_boundary_sizes(const char *who, int Da, int Db, int H, int W, int dilation) {
    if (Da < 0 || Db < 0 || H < 0 || W < 0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: negative size (Da %d, Db %d, H %d, W %d)", who, Da, Db, H, W);
    if (dilation < 1) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: dilation %d < 1", who, dilation);
    if (dilation > kMaxDilation) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "%s: dilation %d > %d", who, dilation, kMaxDilation);
    if ((long long)H * W > 0x7FFFFFFFLL || (long long)H * words_per_row(W) > 0x7FFFFFFFLL)
        return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "%s: %d x %d pixels per mask > 2^31 - 1", who, H, W);
    return 0;
}

}  // namespace

extern "C" size_t mrcnn_mask_iou_workspace_bytes(int Da, int Db, int HW) {
    if (Da < 0 || Db < 0 || HW < 0) return 0;
    return (size_t)((long long)Da + Db) * (size_t)words_per_mask(HW) * sizeof(u64);
}

extern "C" int mrcnn_mask_iou_counts_u8(const unsigned char *a, int Da, const int32_t *a_label, const unsigned char *b, int Db,
                                        const int32_t *b_label, int HW, void *ws, size_t ws_bytes, int32_t *inter, int32_t *area_a,
                                        int32_t *area_b, void *stream) {
    if (Da < 0 || Db < 0 || HW < 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_iou_counts: negative size (Da %d, Db %d, HW %d)", Da, Db, HW);
    if ((a_label == nullptr) != (b_label == nullptr))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_iou_counts: a_label and b_label must be both given or both NULL");
    const long long n_inter = (long long)Da * Db;
    if ((Da > 0 && (!area_a || (HW > 0 && !a))) || (Db > 0 && (!area_b || (HW > 0 && !b))) || (n_inter > 0 && !inter))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_iou_counts: null pointer for a non-empty side");
    const size_t need = mrcnn_mask_iou_workspace_bytes(Da, Db, HW);
    if (ws_bytes < need || (need > 0 && !ws))
        return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "mask_iou_counts: workspace of %zu bytes < %zu", ws_bytes, need);
    const long long NW = words_per_mask(HW);
    const long long ntj = (Db + kTile - 1) / kTile, ntiles = (long long)((Da + kTile - 1) / kTile) * ntj;
    if (ntiles > 0x7FFFFFFFLL) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "mask_iou_counts: %d x %d masks", Da, Db);
    const hipStream_t st = (hipStream_t)stream;
    const long long nzero = n_inter + Da + Db;
    if (nzero == 0) return 0;
    hipLaunchKernelGGL(k_mask_iou_zero, dim3((unsigned)std::min<long long>((nzero + 255) / 256, 1024)), dim3(256), 0, st, area_a, Da, area_b,
                       Db, inter, n_inter);
    MRCNN_LAUNCH_CHECK();
    if (NW == 0) return 0;
    u64 *words = static_cast<u64 *>(ws);
    const long long nmask = (long long)Da + Db, nwin = (NW + 15) / 16;
    const long long gx = std::max(1LL, std::min((nwin + 4 * kUnroll - 1) / (4 * kUnroll), (kTargetBlocks + nmask - 1) / nmask));
    hipLaunchKernelGGL(k_mask_pack, dim3((unsigned)gx, (unsigned)std::min(nmask, 65535LL)), dim3(kPackBlock), 0, st, a, Da, b, Db,
                       (long long)HW, NW, words, area_a, area_b);
    MRCNN_LAUNCH_CHECK();
    if (n_inter == 0) return 0;
    // split the word range so that even one pair fills the chip; ranges are whole LDS stages
    const long long nsplit = std::max(1LL, std::min({(kTargetBlocks + ntiles - 1) / ntiles, (NW + kChunk - 1) / kChunk, 65535LL}));
    const long long wps = ((NW + nsplit - 1) / nsplit + kChunk - 1) / kChunk * kChunk;
    hipLaunchKernelGGL(k_mask_and_popc, dim3((unsigned)ntiles, (unsigned)((NW + wps - 1) / wps)), dim3(kTile * kTile), 0, st, words, Da,
                       words + (size_t)Da * NW, Db, NW, wps, (int)ntj, a_label, b_label, inter);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mrcnn_mask_boundary_workspace_bytes(int Da, int Db, int H, int W) {
    if (Da < 0 || Db < 0 || H < 0 || W < 0) return 0;
    return 2 * (size_t)((long long)Da + Db) * (size_t)H * (size_t)words_per_row(W) * sizeof(u64);
}

extern "C" int mrcnn_mask_boundary_words_u8(const unsigned char *masks, int D, int H, int W, int dilation, void *ws, size_t ws_bytes,
                                            void *bwords, void *stream) {
    if (const int e = check_boundary_sizes("mask_boundary_words", D, 0, H, W, dilation)) return e;
    const size_t nbytes = (size_t)D * (size_t)H * (size_t)words_per_row(W) * sizeof(u64);
    if (nbytes > 0 && (!masks || !bwords)) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_boundary_words: null pointer for a non-empty side");
    const size_t need = mrcnn_mask_boundary_workspace_bytes(D, 0, H, W);
    if (ws_bytes < need || (need > 0 && !ws))
        return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "mask_boundary_words: workspace of %zu bytes < %zu", ws_bytes, need);
    if (nbytes == 0) return 0;
    return launch_boundary_stage(masks, D, nullptr, 0, H, W, dilation, static_cast<u64 *>(ws), static_cast<u64 *>(bwords), nullptr, nullptr,
                                 nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int mrcnn_mask_boundary_iou_counts_u8(const unsigned char *a, int Da, const int32_t *a_label, const unsigned char *b, int Db,
                                                 const int32_t *b_label, int H, int W, int dilation, void *ws, size_t ws_bytes,
                                                 int32_t *inter, int32_t *area_a, int32_t *area_b, int32_t *binter, int32_t *barea_a,
                                                 int32_t *barea_b, void *stream) {
    if (const int e = check_boundary_sizes("mask_boundary_iou_counts", Da, Db, H, W, dilation)) return e;
    if ((a_label == nullptr) != (b_label == nullptr))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_boundary_iou_counts: a_label and b_label must be both given or both NULL");
    const long long n_inter = (long long)Da * Db, HW = (long long)H * W;
    if ((Da > 0 && (!area_a || !barea_a || (HW > 0 && !a))) || (Db > 0 && (!area_b || !barea_b || (HW > 0 && !b))) ||
        (n_inter > 0 && (!inter || !binter)))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_boundary_iou_counts: null pointer for a non-empty side");
    const size_t need = mrcnn_mask_boundary_workspace_bytes(Da, Db, H, W);
    if (ws_bytes < need || (need > 0 && !ws))
        return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "mask_boundary_iou_counts: workspace of %zu bytes < %zu", ws_bytes, need);
    const long long ntj = (Db + kTile - 1) / kTile, ntiles = (long long)((Da + kTile - 1) / kTile) * ntj;
    if (ntiles > 0x7FFFFFFFLL) return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "mask_boundary_iou_counts: %d x %d masks", Da, Db);
    const hipStream_t st = (hipStream_t)stream;
    const long long nzero = n_inter + Da + Db;
    if (nzero == 0) return 0;
    const dim3 gzero((unsigned)std::min<long long>((nzero + 255) / 256, 1024));
    hipLaunchKernelGGL(k_mask_iou_zero, gzero, dim3(256), 0, st, area_a, Da, area_b, Db, inter, n_inter);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mask_iou_zero, gzero, dim3(256), 0, st, barea_a, Da, barea_b, Db, binter, n_inter);
    MRCNN_LAUNCH_CHECK();
    const long long NW = (long long)H * words_per_row(W), nmask = (long long)Da + Db;      // words per mask, row-aligned
    if (NW == 0) return 0;
    u64 *mwords = static_cast<u64 *>(ws), *bwords = mwords + (size_t)nmask * NW;
    if (const int e = launch_boundary_stage(a, Da, b, Db, H, W, dilation, mwords, bwords, area_a, area_b, barea_a, barea_b, st)) return e;
    if (n_inter == 0) return 0;
    // the word split of mrcnn_mask_iou_counts_u8, on the row-aligned words
    const long long nsplit = std::max(1LL, std::min({(kTargetBlocks + ntiles - 1) / ntiles, (NW + kChunk - 1) / kChunk, 65535LL}));
    const long long wps = ((NW + nsplit - 1) / nsplit + kChunk - 1) / kChunk * kChunk;
    const dim3 gpop((unsigned)ntiles, (unsigned)((NW + wps - 1) / wps));
    hipLaunchKernelGGL(k_mask_and_popc, gpop, dim3(kTile * kTile), 0, st, mwords, Da, mwords + (size_t)Da * NW, Db, NW, wps, (int)ntj, a_label,
                       b_label, inter);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mask_and_popc, gpop, dim3(kTile * kTile), 0, st, bwords, Da, bwords + (size_t)Da * NW, Db, NW, wps, (int)ntj, a_label,
                       b_label, binter);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
