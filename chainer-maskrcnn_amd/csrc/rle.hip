// COCO run-length encoding of full-resolution masks on gfx950 (chainer_maskrcnn/evaluator.py InstanceSegmentationCOCOEvaluator,
// evaluate.py): the counts of pycocotools' maskApi.c rleEncode for every mask of a (D, H, W) byte tensor.  Replaces copying the masks
// to the host (30 MB per 480 x 640 image at 100 detections) and scanning them there.
// Runs are taken over the column-major flattening, p = x * H + y; a change is a pixel whose value differs from the pixel before it in
// that order (the value before p = 0 counts as 0), and the counts are the differences of consecutive change positions plus H * W -
// the last one.  Work unit: a segment = 64 rows of one column (rows [64 rb, 64 rb + 64) of column x), one bit per row.
//   tile  : grid (tiles of 64 rows x 256 columns, masks).  The tile's rows are staged in LDS with 16-byte loads of the aligned window
//           that covers them (rows may start at any byte offset), then each wave turns 64 columns into segment words with one ballot
//           per column (lane = row).  change = w ^ (w << 1 | bit before row 0 of the segment).
//           count: per segment (number of changes | pixels set << 8, position of its last change or -1) into the workspace;
//           write: per segment, its changes' differences at their column-major ranks.
//   scan  : one workgroup per mask; exclusive prefix over the mask's segments in column-major order (x, rb) of the change counts
//           (-> the rank of a segment's first change) and of the last positions as a running maximum (-> the position of the change
//           before it, 0 for none); per mask the run count, the position of its last change and its area.
//   offset: one workgroup; exclusive prefix of the run counts over the masks -> offsets.
// No atomics and no hand-off between workgroups inside a launch: every sum has a fixed shape, so the outputs are exact and the same
// from run to run.
#include "common.h"

#include <algorithm>
#include <climits>

namespace {

typedef unsigned long long u64;

constexpr int kBlock = 256;                      // 4 waves
constexpr int kTR = 64;                          // tile rows: one bit per lane of a ballot
constexpr int kTW = 256;                         // tile columns: 64 per wave
constexpr int kChunks = kTW / 16 + 1;            // 16-byte chunks of a row's aligned window
constexpr int kLdsRow = kChunks * 16 + 4;        // LDS bytes per row: the window + 4, so that rows start in different banks

struct MaskTotal {                               // per mask, written by the scan
    int runs;                                    // changes + 1
    int last;                                    // position of the last change (0: none)
};

__device__ __forceinline__ int nrow_blocks(int H) { return (H + kTR - 1) / kTR; }

// The change words of this lane's segment: lane j of wave wv holds column x = x0 + 64 wv + j, rows [y0, y0 + nrows).  Returns false
// for a column past the mask's width (w = c = 0 then).  All threads of the block must call it (it synchronises).
__device__ __forceinline__ bool tile_segments(const unsigned char *__restrict__ m, int d, int H, int W, int x0, int y0,
                                              unsigned char (*tile)[kLdsRow], int *s_off, u64 &w, u64 &c, int &x) {
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int nrows = min(kTR, H - y0), ncols = min(kTW, W - x0);
    const unsigned char *base = m + ((long long)d * H + y0) * W + x0;
    for (int e = t; e < nrows * kChunks; e += kBlock) {
        const int r = e / kChunks, k = e % kChunks;
        const unsigned char *row = base + (long long)r * W;
        const int s = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        if (k == 0) s_off[r] = s;
        // chunk k holds row bytes [16 k - s, 16 k - s + 16); loaded only when it overlaps [0, ncols), so it lies in a 16-byte
        // granule that holds a byte of the row and never leaves the row's pages
        if (16 * k - s < ncols) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row - s + 16 * k);
            unsigned *dst = reinterpret_cast<unsigned *>(&tile[r][16 * k]);
            dst[0] = v.x;
            dst[1] = v.y;
            dst[2] = v.z;
            dst[3] = v.w;
        }
    }
    __syncthreads();
    const bool row_ok = lane < nrows;
    const int so = row_ok ? s_off[lane] : 0;
    w = 0;
#pragma unroll 8
    for (int j = 0; j < kWave; ++j) {
        const int col = wv * kWave + j;
        const bool bit = row_ok && col < ncols && tile[lane][so + col] != 0;
        const u64 b = __ballot(bit);
        if (lane == j) w = b;
    }
    const int col = wv * kWave + lane;
    x = x0 + col;
    c = 0;
    if (col >= ncols) return false;
    unsigned prev = 0;                                                      // the pixel before (y0, x) in column-major order
    if (y0 > 0) prev = m[((long long)d * H + y0 - 1) * W + x] != 0;
    else if (x > 0) prev = m[((long long)d * H + H - 1) * W + x - 1] != 0;
    const u64 valid = nrows == kTR ? ~0ull : (1ull << nrows) - 1;
    c = (w ^ ((w << 1) | prev)) & valid;
    return true;
}

__global__ __launch_bounds__(kBlock) void k_rle_tile_count(const unsigned char *__restrict__ m, int D, int H, int W,
                                                           int2 *__restrict__ seg) {
    __shared__ unsigned char tile[kTR][kLdsRow];
    __shared__ int s_off[kTR];
    const int nrb = nrow_blocks(H);
    const int x0 = (blockIdx.x / nrb) * kTW, rb = blockIdx.x % nrb, y0 = rb * kTR;
    for (int d = blockIdx.y; d < D; d += gridDim.y) {
        u64 w, c;
        int x;
        if (tile_segments(m, d, H, W, x0, y0, tile, s_off, w, c, x)) {
            const int last = c ? x * H + y0 + 63 - __clzll((long long)c) : -1;
            seg[((long long)d * W + x) * nrb + rb] = make_int2(__popcll(c) | (__popcll(w) << 8), last);
        }
        __syncthreads();                                                    // the tile is reused by the next mask
    }
}

// Inclusive scan of (sum, sum2, max) over the block's threads in thread order; *_ex of the block totals and each thread's exclusive
// maximum.  s_* hold kBlock ints.
__device__ __forceinline__ void block_scan(int &sum, int &sum2, int &mx, int &mx_ex, int *s_sum, int *s_sum2, int *s_max, int &tot,
                                           int &tot2, int &tot_max) {
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    for (int o = 1; o < kWave; o <<= 1) {
        const int a = __shfl_up(sum, o), b = __shfl_up(sum2, o), e = __shfl_up(mx, o);
        if (lane >= o) { sum += a; sum2 += b; mx = max(mx, e); }
    }
    if (lane == kWave - 1) { s_sum[wv] = sum; s_sum2[wv] = sum2; s_max[wv] = mx; }
    __syncthreads();
    tot = 0; tot2 = 0; tot_max = INT_MIN;
    int pre = 0, pre2 = 0, pre_max = INT_MIN;
    for (int i = 0; i < kBlock / kWave; ++i) {
        if (i == wv) { pre = tot; pre2 = tot2; pre_max = tot_max; }
        tot += s_sum[i];
        tot2 += s_sum2[i];
        tot_max = max(tot_max, s_max[i]);
    }
    __syncthreads();
    sum += pre;
    sum2 += pre2;
    mx = max(mx, pre_max);
    s_max[t] = mx;
    __syncthreads();
    mx_ex = t ? s_max[t - 1] : INT_MIN;
    __syncthreads();
}

// grid (masks).  Segments of mask d, in column-major order (x, rb): (count | area << 8, last) -> (rank of the segment's first change
// within the mask, position of the change before it or 0).
__global__ __launch_bounds__(kBlock) void k_rle_scan(int D, int H, int W, int2 *__restrict__ seg, MaskTotal *__restrict__ tot_out,
                                                     int32_t *__restrict__ area) {
    __shared__ int s_sum[kBlock / kWave], s_sum2[kBlock / kWave], s_max[kBlock];
    const long long n = (long long)W * nrow_blocks(H);
    for (int d = blockIdx.x; d < D; d += gridDim.x) {
        int2 *sd = seg + (long long)d * n;
        int carry = 0, carry_area = 0, carry_max = 0;                       // no change before: position 0
        for (long long i0 = 0; i0 < n; i0 += kBlock) {
            const long long i = i0 + threadIdx.x;
            const int2 v = i < n ? sd[i] : make_int2(0, -1);
            const int cnt = v.x & 0xFF;
            int sum = cnt, sum2 = v.x >> 8, mx = v.y, mx_ex, tot, tot2, tot_max;
            block_scan(sum, sum2, mx, mx_ex, s_sum, s_sum2, s_max, tot, tot2, tot_max);
            if (i < n) sd[i] = make_int2(carry + sum - cnt, max(carry_max, mx_ex));
            carry += tot;
            carry_area += tot2;
            carry_max = max(carry_max, tot_max);
        }
        if (threadIdx.x == 0) {
            tot_out[d].runs = carry + 1;
            tot_out[d].last = carry_max;
            if (area) area[d] = carry_area;
        }
    }
}

// One workgroup: offsets[d] = sum of runs of the masks before d, offsets[D] = the total.
__global__ __launch_bounds__(kBlock) void k_rle_offsets(int D, const MaskTotal *__restrict__ tot_in, int32_t *__restrict__ offsets) {
    __shared__ int s_sum[kBlock / kWave], s_sum2[kBlock / kWave], s_max[kBlock];
    int carry = 0;
    for (int i0 = 0; i0 < D; i0 += kBlock) {
        const int i = i0 + (int)threadIdx.x;
        const int r = i < D ? tot_in[i].runs : 0;
        int sum = r, sum2 = 0, mx = 0, mx_ex, tot, tot2, tot_max;
        block_scan(sum, sum2, mx, mx_ex, s_sum, s_sum2, s_max, tot, tot2, tot_max);
        if (i < D) offsets[i] = carry + sum - r;
        carry += tot;
    }
    if (threadIdx.x == 0) offsets[D] = carry;
}

__global__ __launch_bounds__(kBlock) void k_rle_tile_write(const unsigned char *__restrict__ m, int D, int H, int W,
                                                           const int2 *__restrict__ seg, const MaskTotal *__restrict__ tot_in,
                                                           const int32_t *__restrict__ offsets, int32_t *__restrict__ counts) {
    __shared__ unsigned char tile[kTR][kLdsRow];
    __shared__ int s_off[kTR];
    const int nrb = nrow_blocks(H);
    const int x0 = nrb ? (blockIdx.x / nrb) * kTW : 0, rb = nrb ? blockIdx.x % nrb : 0, y0 = rb * kTR;
    const bool work = x0 < W && y0 < H;                                     // (H * W == 0: one empty tile per mask)
    for (int d = blockIdx.y; d < D; d += gridDim.y) {
        const int o = offsets[d];
        if (blockIdx.x == 0 && threadIdx.x == 0)                            // the last run: from the last change to the end
            counts[o + tot_in[d].runs - 1] = H * W - tot_in[d].last;
        if (!work) continue;
        u64 w, c;
        int x;
        if (tile_segments(m, d, H, W, x0, y0, tile, s_off, w, c, x) && c) {
            const int2 v = seg[((long long)d * W + x) * nrb + rb];
            const int end = offsets[d + 1] - 1;                             // the mask's last run; masks changed since count cannot
            int prev = v.y;                                                 // write past it
            const int p0 = x * H + y0;
            for (int k = o + v.x; c && k < end; ++k, c &= c - 1) {
                const int q = p0 + __ffsll((long long)c) - 1;
                counts[k] = q - prev;
                prev = q;
            }
        }
        __syncthreads();
    }
}

long long segments_per_mask(int H, int W) { return (long long)W * ((H + kTR - 1) / kTR); }

size_t totals_bytes(int D) { return ((size_t)D * sizeof(MaskTotal) + 255) / 256 * 256; }

// H * W and the worst case of D * (H * W + 1) runs fit int32
bool fits(int D, int H, int W) {
    const long long hw = (long long)H * W;
    return hw <= INT_MAX && (long long)D * (hw + 1) <= INT_MAX;
}

unsigned tiles_per_mask(int H, int W) {
    const long long t = (long long)((W + kTW - 1) / kTW) * ((H + kTR - 1) / kTR);
    return (unsigned)std::max(1LL, t);
}

}  // namespace

extern "C" size_t mrcnn_mask_rle_workspace_bytes(int D, int H, int W) {
    if (D < 0 || H < 0 || W < 0) return 0;
    return totals_bytes(D) + (size_t)D * (size_t)segments_per_mask(H, W) * sizeof(int2);
}

extern "C" int mrcnn_mask_rle_count_u8(const unsigned char *m, int D, int H, int W, void *ws, size_t ws_bytes, int32_t *offsets,
                                       int32_t *area, void *stream) {
    if (D < 0 || H < 0 || W < 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_rle_count: negative size (D %d, H %d, W %d)", D, H, W);
    if (!offsets || (D > 0 && (long long)H * W > 0 && !m))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_rle_count: null pointer for a non-empty side");
    if (!fits(D, H, W))
        return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "mask_rle_count: %d masks of %d x %d pixels: the run total may not fit int32", D, H, W);
    const size_t need = mrcnn_mask_rle_workspace_bytes(D, H, W);
    if (ws_bytes < need || (need > 0 && !ws))
        return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "mask_rle_count: workspace of %zu bytes < %zu", ws_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    MaskTotal *tot = static_cast<MaskTotal *>(ws);
    int2 *seg = reinterpret_cast<int2 *>(static_cast<char *>(ws) + totals_bytes(D));
    if (D > 0) {
        if ((long long)H * W > 0) {
            hipLaunchKernelGGL(k_rle_tile_count, dim3(tiles_per_mask(H, W), (unsigned)std::min(D, 65535)), dim3(kBlock), 0, st, m, D, H, W,
                               seg);
            MRCNN_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_rle_scan, dim3((unsigned)D), dim3(kBlock), 0, st, D, H, W, seg, tot, area);
        MRCNN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_rle_offsets, dim3(1), dim3(kBlock), 0, st, D, tot, offsets);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_mask_rle_write_u8(const unsigned char *m, int D, int H, int W, const void *ws, size_t ws_bytes, const int32_t *offsets,
                                       int32_t *counts, void *stream) {
    if (D < 0 || H < 0 || W < 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_rle_write: negative size (D %d, H %d, W %d)", D, H, W);
    if (D > 0 && (!offsets || !counts || ((long long)H * W > 0 && !m)))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "mask_rle_write: null pointer for a non-empty side");
    if (!fits(D, H, W))
        return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "mask_rle_write: %d masks of %d x %d pixels: the run total may not fit int32", D, H, W);
    const size_t need = mrcnn_mask_rle_workspace_bytes(D, H, W);
    if (ws_bytes < need || (need > 0 && !ws))
        return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "mask_rle_write: workspace of %zu bytes < %zu", ws_bytes, need);
    if (D == 0) return 0;
    const MaskTotal *tot = static_cast<const MaskTotal *>(ws);
    const int2 *seg = reinterpret_cast<const int2 *>(static_cast<const char *>(ws) + totals_bytes(D));
    hipLaunchKernelGGL(k_rle_tile_write, dim3(tiles_per_mask(H, W), (unsigned)std::min(D, 65535)), dim3(kBlock), 0, (hipStream_t)stream, m,
                       D, H, W, seg, tot, offsets, counts);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
