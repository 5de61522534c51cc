// Keypoint heat-map decode on gfx950 (MaskRCNN.predict_keypoints, chainer_maskrcnn/evaluator.py KeypointCOCOEvaluator): for every
// detection d and keypoint k, the argmax over the S x S cells of channel k of the keypoint branch's output, its image position,
// its logit and the softmax probability of that cell.  Replaces the host NumPy of the reference's viewer.py:86-107 (argmax of
// predict()'s (D, K, S*S) heat maps, mapped into the box).
//   partial : grid (split, detection).  Each workgroup reduces a contiguous range of cells of one detection to one
//             (max, first index, sum exp(l - max)) triple per keypoint, written to the workspace in (d, k, split) order.
//             HBM-bound: NHWC, so a 16-byte load holds 4 channels of one cell; P = pow2 >= ceil(K/4) lanes per cell, lanes of equal
//             channels are reduced with shuffles, the 4 waves through LDS.
//   merge   : one wave per (d, k) folds its partials (lanes over splits, then a lane butterfly) and writes (y, x, logit, prob) and
//             the index.
// Every reduction has a fixed shape (lane butterflies, waves 0..3, splits by lane), so the result is bit-identical from run to run.
#include "common.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int kBlock = 256;                      // 4 waves
constexpr int kUnroll = 4;                       // cells per thread and step (loads in flight)
constexpr int kTargetBlocks = 2048;              // enough workgroups to fill 256 CUs several times over
constexpr int kMinCellsPerThread = 2;            // below this a split costs more in reductions than it saves in loads

struct Partial {                                 // 16 bytes: one (d, k, split) of the workspace
    float m;                                     // max logit (-inf: no cell seen)
    int idx;                                     // first flat cell index of the max (INT_MAX: no cell seen)
    double s;                                    // sum over the cells seen of exp(l - m)
};

// (m, i, s) <- (m, i, s) (+) (mb, ib, sb).  Larger max wins, equal maxima keep the smaller index (np.argmax's first maximum); the
// sums are rescaled to the common max in double.  Empty operands (s == 0) are neutral.
__device__ __forceinline__ void merge(float &m, int &i, double &s, float mb, int ib, double sb) {
    if (sb == 0.0) return;
    if (s == 0.0) { m = mb; i = ib; s = sb; return; }
    const float M = fmaxf(m, mb);
    const int I = m > mb ? i : (mb > m ? ib : min(i, ib));
    s = s * exp((double)m - (double)M) + sb * exp((double)mb - (double)M);
    m = M;
    i = I;
}

// One cell's logit v at flat index c into a thread's running state; cells arrive in increasing c, so > keeps the first maximum.
__device__ __forceinline__ void update(float &m, int &i, double &s, float v, int c) {
    if (v > m) {
        s = (s == 0.0 ? 0.0 : s * exp((double)m - (double)v)) + 1.0;
        m = v;
        i = c;
    } else {
        s += (double)expf(v - m);
    }
}

// grid (x: splits of the S*S cells, y: detections).  Thread t: lane group g = lane % P reads channels [4g, 4g + 4) of cell
// c0 + (t / P) + (256 / P) * j; lanes with 4g >= K load nothing.
__global__ __launch_bounds__(kBlock) void k_keypoint_partial(const float *__restrict__ heat, int D, int SS, int Cp, int K, int P,
                                                             int cells_per_split, int nsplit, Partial *__restrict__ part) {
    __shared__ double s_s[kBlock / kWave][4 * kWave];     // per wave, channel 4g + j of lane g < P (K <= 4 * 64)
    __shared__ float s_m[kBlock / kWave][4 * kWave];
    __shared__ int s_i[kBlock / kWave][4 * kWave];
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int g = lane & (P - 1), k0 = 4 * g;
    const int step = kBlock / P;                 // cells per block and step
    const bool active = k0 < K;
    const int split = blockIdx.x;
    const int c_begin = split * cells_per_split, c_end = min(SS, c_begin + cells_per_split);
    for (int d = blockIdx.y; d < D; d += gridDim.y) {
        const float *base = heat + (size_t)d * SS * Cp + k0;
        float m[4];
        int idx[4];
        double s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; idx[j] = INT_MAX; s[j] = 0.0; }
        if (active) {
            for (int c0 = c_begin + t / P; c0 < c_end; c0 += kUnroll * step) {
                float4 v[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int c = c0 + u * step;
                    v[u] = c < c_end ? *reinterpret_cast<const float4 *>(base + (size_t)c * Cp) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int c = c0 + u * step;
                    if (c < c_end) {
                        update(m[0], idx[0], s[0], v[u].x, c);
                        update(m[1], idx[1], s[1], v[u].y, c);
                        update(m[2], idx[2], s[2], v[u].z, c);
                        update(m[3], idx[3], s[3], v[u].w, c);
                    }
                }
            }
        }
        // lanes g, g + P, g + 2P, ... hold the same channels: butterfly over the cell bits of the lane id
        for (int mask = P; mask < kWave; mask <<= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float mb = __shfl_xor(m[j], mask);
                const int ib = __shfl_xor(idx[j], mask);
                const double sb = __shfl_xor(s[j], mask);
                merge(m[j], idx[j], s[j], mb, ib, sb);
            }
        }
        if (lane < P) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s_m[wv][4 * lane + j] = m[j];
                s_i[wv][4 * lane + j] = idx[j];
                s_s[wv][4 * lane + j] = s[j];
            }
        }
        __syncthreads();
        if (t < K) {                             // channel t: waves in order 0..3
            float M = s_m[0][t];
            int I = s_i[0][t];
            double S = s_s[0][t];
            for (int w = 1; w < kBlock / kWave; ++w) merge(M, I, S, s_m[w][t], s_i[w][t], s_s[w][t]);
            part[((size_t)d * K + t) * nsplit + split] = Partial{M, I, S};
        }
        __syncthreads();
    }
}

// One wave per (d, k): lane l folds partials l, l + 64, ... in order, then a butterfly over the lanes (a fixed shape: deterministic).
// y = float(idx / S) * ((y2 - y1) / S) + y1 and x likewise, in float32 without contraction (the library is built with
// -ffp-contract=off): the reference viewer's rule (viewer.py:103-106), the inverse of the training target's floor((kp - y0) / h * S)
// (proposal_target_creator.py:111-124) - the TOP-LEFT corner of the cell, not its centre.
__global__ __launch_bounds__(256) void k_keypoint_merge(const Partial *__restrict__ part, int D, int K, int S, int nsplit,
                                                        const float *__restrict__ bbox, float *__restrict__ out,
                                                        int32_t *__restrict__ index) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long n = (long long)D * K, waves = (long long)gridDim.x * (blockDim.x / kWave);
    for (long long e = (long long)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave; e < n; e += waves) {
        const Partial *p = part + e * nsplit;
        float m = -INFINITY;
        int i = INT_MAX;
        double s = 0.0;
        for (int q = lane; q < nsplit; q += kWave) merge(m, i, s, p[q].m, p[q].idx, p[q].s);
        for (int mask = 1; mask < kWave; mask <<= 1) {
            const float mb = __shfl_xor(m, mask);
            const int ib = __shfl_xor(i, mask);
            const double sb = __shfl_xor(s, mask);
            merge(m, i, s, mb, ib, sb);
        }
        if (lane == 0) {
            const long long d = e / K;
            const float y1 = bbox[4 * d + 0], x1 = bbox[4 * d + 1], y2 = bbox[4 * d + 2], x2 = bbox[4 * d + 3];
            const float fs = (float)S;
            const float cy = (float)(i / S), cx = (float)(i % S);
            float4 r;
            r.x = cy * ((y2 - y1) / fs) + y1;
            r.y = cx * ((x2 - x1) / fs) + x1;
            r.z = m;
            r.w = (float)(1.0 / s);
            reinterpret_cast<float4 *>(out)[e] = r;
            if (index) index[e] = i;
        }
    }
}

int lanes_per_cell(int K) {
    int P = 1;
    while (4 * P < K) P <<= 1;
    return P;
}

int n_splits(int D, int S, int K) {
    const long long SS = (long long)S * S;
    const int step = kBlock / lanes_per_cell(K);
    const long long max_split = std::max(1LL, SS / ((long long)step * kMinCellsPerThread));
    const long long want = (kTargetBlocks + (long long)D - 1) / std::max(D, 1);
    return (int)std::max(1LL, std::min(want, max_split));
}

}  // namespace

extern "C" size_t mrcnn_keypoint_decode_workspace_bytes(int D, int S, int K) {
    if (D <= 0 || S <= 0 || K <= 0 || K > 4 * kWave || S > 46340) return 0;
    return (size_t)D * (size_t)K * (size_t)n_splits(D, S, K) * sizeof(Partial);
}

extern "C" int mrcnn_keypoint_decode_f32(const float *heat, int D, int S, int Cp, int K, const float *bbox, void *ws, size_t ws_bytes,
                                         float *out, int32_t *index, void *stream) {
    if (D < 0 || S <= 0 || K <= 0 || Cp < K)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "keypoint_decode: bad sizes (D %d, S %d, Cp %d, K %d)", D, S, Cp, K);
    if (Cp % 4 != 0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "keypoint_decode: channel count Cp %d is not a multiple of 4 (16-byte cell loads)", Cp);
    if (K > 4 * kWave || S > 46340)
        return mrcnn::fail_arg(MRCNN_E_UNSUPPORTED, "keypoint_decode: K %d > %d or S %d > 46340", K, 4 * kWave, S);
    if (D == 0) return 0;
    if (!heat || !bbox || !out) return mrcnn::fail_arg(MRCNN_E_INVALID, "keypoint_decode: null heat, bbox or out pointer");
    if (reinterpret_cast<uintptr_t>(heat) % 16 != 0 || reinterpret_cast<uintptr_t>(out) % 16 != 0)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "keypoint_decode: heat and out must be 16-byte aligned");
    const size_t need = mrcnn_keypoint_decode_workspace_bytes(D, S, K);
    if (ws_bytes < need || !ws) return mrcnn::fail_arg(MRCNN_E_WORKSPACE, "keypoint_decode: workspace of %zu bytes < %zu", ws_bytes, need);
    const int SS = S * S, P = lanes_per_cell(K), nsplit = n_splits(D, S, K);
    const int cells_per_split = (SS + nsplit - 1) / nsplit;
    const hipStream_t st = (hipStream_t)stream;
    Partial *part = static_cast<Partial *>(ws);
    hipLaunchKernelGGL(k_keypoint_partial, dim3((unsigned)nsplit, (unsigned)std::min(D, 65535)), dim3(kBlock), 0, st, heat, D, SS, Cp, K, P,
                       cells_per_split, nsplit, part);
    MRCNN_LAUNCH_CHECK();
    const long long n = (long long)D * K;
    hipLaunchKernelGGL(k_keypoint_merge, dim3((unsigned)std::min<long long>((n + 3) / 4, 4096)), dim3(256), 0, st, part, D, K, S, nsplit,
                       bbox, out, index);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
