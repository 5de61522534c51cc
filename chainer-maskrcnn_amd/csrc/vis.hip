// Rendering of detections on gfx950 (chainer_maskrcnn/vis.py, demo.py): one image (3,H,W) float32 plus its D instances (masks (D,H,W)
// bytes, boxes, colours) plus a list of primitives -> one (H,W,3) uint8 picture.  Replaces copying the (D,H,W) masks to the host
// (100 MB for 100 detections at 800 x 1333) and compositing there: every mask byte is read once and one picture goes back.
// The picture is a pure function of the inputs, in integer arithmetic only, per pixel, painter's order:
//   c = min(255, max(0, floor(v + 0.5))) of the image (NaN -> 0);
//   for d = order[0], .., order[D-1] (0..D-1 without an order): mask[d] set -> c = blend(c, colour[d], mask_a); contour pixel of
//                   mask[d] -> c = colour[d]; on the outline of box d -> c = colour[d];
//   for every primitive in array order: pixel on it -> c = blend(c, its colour, its a).
//   blend(c, col, a) = (c * (256 - a) + col * a + 128) >> 8 per channel, a in [0, 256].
// Work unit: a tile of kTH rows x kTW columns per workgroup, 4 consecutive pixels of a row per thread.  Per instance the tile's mask
// bytes and a one-pixel halo (zero outside the image) are staged in LDS as words - aligned 4-byte loads where the row's address allows,
// two aligned words shifted together where it does not, bytes at the buffer's ends - so that the contour test reads LDS, and a thread
// takes its 4 pixels and their 4-neighbours from five LDS words.  Two LDS buffers alternate: one barrier per instance.  Primitives are
// taken in chunks of kPrimChunk; a chunk's primitives whose bounding box meets the tile are compacted into LDS in array order and only
// those are tested per pixel.  No atomics, no hand-off between workgroups: the same input gives the same bytes on every run.
#include "common.h"

#include <algorithm>

namespace {

constexpr int kBlock = 256;                      // 4 waves
constexpr int kTW = 128;                         // tile columns: 32 threads x 4 pixels
constexpr int kTH = 8;                           // tile rows
constexpr int kRowWords = kTW / 4 + 2;           // a staged row: the tile's words and one halo word on each side
constexpr int kRowStride = kRowWords + 1;        // odd: the rows of a wave start in different banks
constexpr int kTileWords = (kTH + 2) * kRowStride;
constexpr int kInstChunk = 128;                  // instances whose integer boxes and colours are staged at a time
constexpr int kPrimChunk = 256;                  // primitives examined at a time: one per thread

constexpr int kCoordMin = MRCNN_VIS_COORD_MIN, kCoordMax = MRCNN_VIS_COORD_MAX, kParamMax = MRCNN_VIS_PARAM_MAX;

struct Inst {
    int top, left, bottom, right;                // the box outline's corners, inclusive
    unsigned rgb;
    int src;                                     // the instance drawn at this place of the order, -1: none
};

// floor(v + 0.5) clamped into the coordinate range (NaN -> the lower end)
__device__ __forceinline__ int round_coord(float v) {
    const float q = floorf(v + 0.5f);
    return q >= (float)kCoordMax ? kCoordMax : (q > (float)kCoordMin ? (int)q : kCoordMin);
}

__device__ __forceinline__ unsigned round_u8(float v) {
    const float q = floorf(v + 0.5f);
    return q >= 255.0f ? 255u : (q > 0.0f ? (unsigned)q : 0u);
}

// packed colours: r | g << 8 | b << 16
__device__ __forceinline__ unsigned blend(unsigned c, unsigned col, unsigned a) {
    if (a == 256u) return col;
    const unsigned na = 256u - a;
    const unsigned r = ((c & 0xFF) * na + (col & 0xFF) * a + 128u) >> 8;
    const unsigned g = (((c >> 8) & 0xFF) * na + ((col >> 8) & 0xFF) * a + 128u) >> 8;
    const unsigned b = (((c >> 16) & 0xFF) * na + ((col >> 16) & 0xFF) * a + 128u) >> 8;
    return r | (g << 8) | (b << 16);
}

// bit i = byte i of w is nonzero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {
    const unsigned t = ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7;
    return (t | (t >> 7) | (t >> 14) | (t >> 21)) & 15u;
}

// The tile of one mask plane (m_plane = the plane's first byte) with its halo into LDS: word k of row r holds the pixels
// x0 - 4 + 4 k .. + 3 of image row y0 - 1 + r, zero outside the image.  [m_lo, m_hi) is the whole mask buffer: no load leaves it.
__device__ __forceinline__ void stage_mask(const unsigned char *__restrict__ m_plane, const unsigned char *m_lo, const unsigned char *m_hi,
                                           int H, int W, int x0, int y0, unsigned *tile) {
    for (int e = threadIdx.x; e < (kTH + 2) * kRowWords; e += kBlock) {
        const int r = e / kRowWords, k = e % kRowWords;
        const int y = y0 - 1 + r, x = x0 - 4 + 4 * k;
        unsigned w = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const unsigned char *p = m_plane + (long long)y * W + x;
            if (x + 3 < W) {
                const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
                const unsigned char *q = p - sh;
                if (sh == 0)
                    w = *reinterpret_cast<const unsigned *>(q);
                else if (q >= m_lo && q + 8 <= m_hi)
                    w = (reinterpret_cast<const unsigned *>(q)[0] >> (8 * sh)) | (reinterpret_cast<const unsigned *>(q)[1] << (32 - 8 * sh));
                else
                    w = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
            } else {
                for (int i = 0; i < 4; ++i)
                    if (x + i < W) w |= (unsigned)p[i] << (8 * i);
            }
        }
        tile[r * kRowStride + k] = w;
    }
}

struct Prim {                                    // mrcnn_vis_prim_t as staged: a glyph carries its bitmap in x1 (low) and y1 (high)
    int kind, x0, y0, x1, y1, p;
    unsigned rgb, a;
};

__device__ __forceinline__ bool coord_ok(int v) { return v >= kCoordMin && v <= kCoordMax; }

// The primitive's bounding box (inclusive) when it is well formed, false otherwise (such a primitive draws nothing).
__device__ __forceinline__ bool prim_bounds(const Prim &q, int &bx0, int &by0, int &bx1, int &by1) {
    if (!coord_ok(q.x0) || !coord_ok(q.y0) || q.a > 256u || q.p < 0 || q.p > kParamMax) return false;
    switch (q.kind) {
    case MRCNN_VIS_RECT:
    case MRCNN_VIS_FILL:
        if (!coord_ok(q.x1) || !coord_ok(q.y1) || (q.kind == MRCNN_VIS_RECT && q.p < 1)) return false;
        bx0 = q.x0; by0 = q.y0; bx1 = q.x1; by1 = q.y1;
        return true;
    case MRCNN_VIS_SEGMENT:
        if (!coord_ok(q.x1) || !coord_ok(q.y1)) return false;
        bx0 = min(q.x0, q.x1) - q.p; bx1 = max(q.x0, q.x1) + q.p;
        by0 = min(q.y0, q.y1) - q.p; by1 = max(q.y0, q.y1) + q.p;
        return true;
    case MRCNN_VIS_DISC:
        bx0 = q.x0 - q.p; bx1 = q.x0 + q.p; by0 = q.y0 - q.p; by1 = q.y0 + q.p;
        return true;
    case MRCNN_VIS_GLYPH:
        if (q.p < 1 || q.p > MRCNN_VIS_GLYPH_SCALE_MAX) return false;
        bx0 = q.x0; by0 = q.y0; bx1 = q.x0 + MRCNN_VIS_GLYPH_W * q.p - 1; by1 = q.y0 + MRCNN_VIS_GLYPH_H * q.p - 1;
        return true;
    default:
        return false;
    }
}

__device__ __forceinline__ bool on_outline(int x, int y, int left, int top, int right, int bottom, int t) {
    return x >= left && x <= right && y >= top && y <= bottom && (x < left + t || x > right - t || y < top + t || y > bottom - t);
}

// pixel (x, y) on the primitive; the caller has checked the bounding box
__device__ __forceinline__ bool on_prim(const Prim &q, int x, int y) {
    switch (q.kind) {
    case MRCNN_VIS_FILL:
        return true;
    case MRCNN_VIS_RECT:
        return on_outline(x, y, q.x0, q.y0, q.x1, q.y1, q.p);
    case MRCNN_VIS_DISC: {
        const long long dx = x - q.x0, dy = y - q.y0;
        return dx * dx + dy * dy <= (long long)q.p * q.p;
    }
    case MRCNN_VIS_SEGMENT: {
        const long long dx = q.x1 - q.x0, dy = q.y1 - q.y0, wx = x - q.x0, wy = y - q.y0;
        const long long L = dx * dx + dy * dy, s = wx * dx + wy * dy, t2 = (long long)q.p * q.p;
        if (L == 0 || s <= 0) return 4 * (wx * wx + wy * wy) <= t2;
        if (s >= L) {
            const long long ex = x - q.x1, ey = y - q.y1;
            return 4 * (ex * ex + ey * ey) <= t2;
        }
        const long long cr = wx * dy - wy * dx;
        return 4 * cr * cr <= t2 * L;
    }
    default: {                                   // MRCNN_VIS_GLYPH
        const int col = (x - q.x0) / q.p, row = (y - q.y0) / q.p, bit = row * MRCNN_VIS_GLYPH_W + col;
        return ((bit < 32 ? (unsigned)q.x1 >> bit : (unsigned)q.y1 >> (bit - 32)) & 1u) != 0;
    }
    }
}

// grid (tiles along x, tiles along y)
__global__ __launch_bounds__(kBlock) void k_vis_render(const float *__restrict__ img, int H, int W, const unsigned char *__restrict__ masks,
                                                       const float *__restrict__ bbox, const unsigned char *__restrict__ colors,
                                                       const int32_t *__restrict__ order, int D, unsigned mask_a, int box_t, int flags,
                                                       const mrcnn_vis_prim_t *__restrict__ prims, int n_prims,
                                                       const unsigned long long *__restrict__ font, int n_glyphs,
                                                       unsigned char *__restrict__ out) {
    __shared__ unsigned s_tile[2][kTileWords];
    __shared__ Inst s_inst[kInstChunk];
    __shared__ Prim s_prim[kPrimChunk];
    __shared__ int s_cnt[kBlock / kWave];
    const int t = threadIdx.x, tx = t % (kTW / 4), ty = t / (kTW / 4);
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int x = x0 + 4 * tx, y = y0 + ty;
    const bool live = x < W && y < H;
    const long long hw = (long long)H * W;

    unsigned px[4] = {0, 0, 0, 0};
    if (live) {
        const long long idx = (long long)y * W + x;
        for (int c = 0; c < 3; ++c) {
            const float *p = img + c * hw + idx;
            if (x + 3 < W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                const float4 v = *reinterpret_cast<const float4 *>(p);
                px[0] |= round_u8(v.x) << (8 * c);
                px[1] |= round_u8(v.y) << (8 * c);
                px[2] |= round_u8(v.z) << (8 * c);
                px[3] |= round_u8(v.w) << (8 * c);
            } else {
                for (int i = 0; i < 4; ++i)
                    if (x + i < W) px[i] |= round_u8(p[i]) << (8 * c);
            }
        }
    }

    const bool use_masks = (flags & (MRCNN_VIS_DRAW_MASKS | MRCNN_VIS_DRAW_CONTOURS)) != 0;
    const bool draw_boxes = (flags & MRCNN_VIS_DRAW_BOXES) != 0;
    const unsigned char *m_hi = masks + (long long)D * hw;
    int buf = 0;
    for (int d0 = 0; d0 < D; d0 += kInstChunk) {
        const int nd = min(kInstChunk, D - d0);
        __syncthreads();                         // the previous chunk's instances have been read
        if (t < nd) {
            Inst in;
            in.src = order ? order[d0 + t] : d0 + t;
            if (in.src < 0 || in.src >= D) in.src = -1;                     // an index outside the instances draws nothing
            in.top = in.left = 0;
            in.bottom = in.right = -1;           // an empty outline when boxes are not drawn
            in.rgb = 0;
            if (in.src >= 0) {
                if (draw_boxes) {
                    const float *b = bbox + 4ll * in.src;
                    in.top = round_coord(b[0]); in.left = round_coord(b[1]); in.bottom = round_coord(b[2]); in.right = round_coord(b[3]);
                }
                const unsigned char *c = colors + 3ll * in.src;
                in.rgb = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
            }
            s_inst[t] = in;
        }
        __syncthreads();
        for (int j = 0; j < nd; ++j) {
            const Inst in = s_inst[j];
            unsigned set = 0, contour = 0;
            if (use_masks && in.src >= 0) {      // (the same in every thread)
                unsigned *tile = s_tile[buf];    // written here, read after the barrier; last read before the previous barrier
                buf ^= 1;
                stage_mask(masks + in.src * hw, masks, m_hi, H, W, x0, y0, tile);
                __syncthreads();
                const unsigned *row = tile + (ty + 1) * kRowStride + tx + 1;
                const unsigned wc = row[0];
                if (wc) {
                    set = nonzero_bytes(wc);
                    const unsigned up = nonzero_bytes(row[-kRowStride]), down = nonzero_bytes(row[kRowStride]);
                    const unsigned lf = ((set << 1) | ((row[-1] >> 24) != 0)) & 15u;
                    const unsigned rt = (set >> 1) | (((row[1] & 0xFFu) != 0) << 3);
                    contour = set & ~(up & down & lf & rt);
                }
            }
            const bool in_y = y >= in.top && y <= in.bottom;
            const bool edge_y = y < in.top + box_t || y > in.bottom - box_t;
            if (!(flags & MRCNN_VIS_DRAW_MASKS)) set = 0;
            if (!(flags & MRCNN_VIS_DRAW_CONTOURS)) contour = 0;
            if (set | contour | (unsigned)in_y) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xi = x + i;
                    if ((set >> i) & 1u) px[i] = blend(px[i], in.rgb, mask_a);
                    if ((contour >> i) & 1u) px[i] = in.rgb;
                    if (in_y && xi >= in.left && xi <= in.right && (edge_y || xi < in.left + box_t || xi > in.right - box_t)) px[i] = in.rgb;
                }
            }
        }
    }

    // primitives: compact the chunk's primitives that meet this tile into LDS, in array order
    const int lane = t & (kWave - 1), wv = t / kWave;
    const int tx1 = min(x0 + kTW, W) - 1, ty1 = min(y0 + kTH, H) - 1;
    for (int p0 = 0; p0 < n_prims; p0 += kPrimChunk) {
        Prim q;
        bool hit = false;
        if (p0 + t < n_prims) {
            const int4 *src = reinterpret_cast<const int4 *>(prims + p0 + t);
            const int4 a = src[0], b = src[1];
            q.kind = a.x; q.x0 = a.y; q.y0 = a.z; q.x1 = a.w; q.y1 = b.x; q.p = b.y; q.rgb = (unsigned)b.z & 0xFFFFFFu; q.a = (unsigned)b.w;
            int bx0, by0, bx1, by1;
            hit = prim_bounds(q, bx0, by0, bx1, by1) && bx0 <= tx1 && bx1 >= x0 && by0 <= ty1 && by1 >= y0;
            if (hit && q.kind == MRCNN_VIS_GLYPH) {                       // an index outside the font: a filled cell
                const unsigned long long bits = q.x1 >= 0 && q.x1 < n_glyphs ? font[q.x1] : ~0ull;
                q.x1 = (int)(unsigned)bits;
                q.y1 = (int)(unsigned)(bits >> 32);
            }
        }
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();                         // also: the previous chunk's s_prim has been read
        int off = 0, total = 0;
        for (int i = 0; i < kBlock / kWave; ++i) {
            if (i < wv) off += s_cnt[i];
            total += s_cnt[i];
        }
        if (hit) s_prim[off + __popcll(bal & ((1ull << lane) - 1))] = q;
        __syncthreads();
        for (int i = 0; i < total; ++i) {
            const Prim pq = s_prim[i];
            int bx0, by0, bx1, by1;
            prim_bounds(pq, bx0, by0, bx1, by1);
            if (y < by0 || y > by1 || x > bx1 || x + 3 < bx0) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xi = x + k;
                if (xi >= bx0 && xi <= bx1 && on_prim(pq, xi, y)) px[k] = blend(px[k], pq.rgb, pq.a);
            }
        }
        __syncthreads();                         // s_cnt and s_prim are rewritten by the next chunk
    }

    if (!live) return;
    unsigned char *o = out + 3 * ((long long)y * W + x);
    if (x + 3 < W && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        unsigned *ow = reinterpret_cast<unsigned *>(o);
        ow[0] = px[0] | (px[1] << 24);
        ow[1] = (px[1] >> 8) | (px[2] << 16);
        ow[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int i = 0; i < 4; ++i)
            if (x + i < W) {
                o[3 * i] = (unsigned char)px[i];
                o[3 * i + 1] = (unsigned char)(px[i] >> 8);
                o[3 * i + 2] = (unsigned char)(px[i] >> 16);
            }
    }
}

}  // namespace

extern "C" int mrcnn_vis_render_u8(const float *img, int H, int W, const unsigned char *masks, const float *bbox, const unsigned char *colors,
                                   const int32_t *order, int D, int mask_a256, int box_thickness, int flags, const mrcnn_vis_prim_t *prims, int n_prims,
                                   const unsigned long long *font, int n_glyphs, unsigned char *out, void *stream) {
    static_assert(sizeof(mrcnn_vis_prim_t) == 32, "mrcnn_vis_prim_t is 8 int32");
    if (H < 0 || H > MRCNN_VIS_MAX_SIDE) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: H %d outside 0..%d", H, MRCNN_VIS_MAX_SIDE);
    if (W < 0 || W > MRCNN_VIS_MAX_SIDE) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: W %d outside 0..%d", W, MRCNN_VIS_MAX_SIDE);
    if (D < 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: D %d is negative", D);
    if (n_prims < 0) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: n_prims %d is negative", n_prims);
    if (n_glyphs < 0 || n_glyphs > MRCNN_VIS_GLYPHS_MAX)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: n_glyphs %d outside 0..%d", n_glyphs, MRCNN_VIS_GLYPHS_MAX);
    if (flags & ~(MRCNN_VIS_DRAW_MASKS | MRCNN_VIS_DRAW_CONTOURS | MRCNN_VIS_DRAW_BOXES))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: flags 0x%x has unknown bits", flags);
    if (mask_a256 < 0 || mask_a256 > 256) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: mask_a256 %d outside 0..256", mask_a256);
    if (box_thickness < 1 || box_thickness > MRCNN_VIS_PARAM_MAX)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: box_thickness %d outside 1..%d", box_thickness, MRCNN_VIS_PARAM_MAX);
    const bool pixels = (long long)H * W > 0;
    if (pixels && !img) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: img is NULL");
    if (pixels && !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: out is NULL");
    if (D > 0 && !colors) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: colors is NULL for %d instances", D);
    if (D > 0 && pixels && (flags & (MRCNN_VIS_DRAW_MASKS | MRCNN_VIS_DRAW_CONTOURS)) && !masks)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: masks is NULL although masks or contours are drawn");
    if (D > 0 && (flags & MRCNN_VIS_DRAW_BOXES) && !bbox) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: bbox is NULL although boxes are drawn");
    if (n_prims > 0 && (!prims || (reinterpret_cast<uintptr_t>(prims) & 15)))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: prims is NULL or not 16-byte aligned");
    if (n_glyphs > 0 && (!font || (reinterpret_cast<uintptr_t>(font) & 7)))
        return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: font is NULL or not 8-byte aligned");
    if (order && (reinterpret_cast<uintptr_t>(order) & 3)) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: order is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(img) & 3) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: img is not 4-byte aligned");
    if (bbox && (reinterpret_cast<uintptr_t>(bbox) & 3)) return mrcnn::fail_arg(MRCNN_E_INVALID, "vis_render: bbox is not 4-byte aligned");
    if (!pixels) return 0;
    const dim3 grid((unsigned)mrcnn::cdiv(W, kTW), (unsigned)mrcnn::cdiv(H, kTH));
    hipLaunchKernelGGL(k_vis_render, grid, dim3(kBlock), 0, (hipStream_t)stream, img, H, W, masks, bbox, colors, order, D, (unsigned)mask_a256,
                       box_thickness, flags, prims, n_prims, font, n_glyphs, out);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
