// The optimizer side of the training recipe over the flat buffers (gfx950, fp32): gradient accumulation over micro-batches, the global
// gradient norm for clipping, and the MomentumSGD + WeightDecay update whose learning rate and gradient scale live ON THE DEVICE.
//
//   k_accumulate   acc = g (first micro-batch) or acc = acc + g.                                             8 / 12 B per trainable parameter
//   k_sqnorm       per-block partial sums of (acc + g)^2 (or g^2), every square and every sum in double.     8 / 4 B
//   k_norm_finish  one block: the partials in a fixed order -> norm, rate, scale in the hyper block.
//   k_sgd_hyper    ge = acc + g (or g); gs = ge * scale; v = momentum*v - lr*(gs + wd*p); p += v             24 / 20 B
//                  with lr = hyper[HYPER_LR] and scale = hyper[HYPER_SCALE] read from the device.
//
// All are float4 streaming kernels in the manner of k_sgd_masked (bn_frozen.hip): a section [0, n) whose first element is element
// `offset` of the flat buffer, float4 groups aligned to the FLAT buffer, the up to 3 elements in front of the first group and behind the
// last one go one by one; 64-float blocks whose bit is set in `frozen` are neither read nor written (frozen == nullptr: nothing is frozen).
// No atomics, no host synchronisation: the sum of squares is taken on a grid that depends on n alone, block b writes partial b, the
// finishing block adds the partials in index order - the same bits on every run.
//
// Hyper block (MRCNN_HYPER_FLOATS floats, owned by the optimizer): [0] lr, [1] a (1 or 1/k), [2] clip threshold - placed by the host;
// [3] scale, [4] norm, [5] rate - written by k_norm_finish (scale also by the host when no norm is taken); [6] the number of skipped
// updates as a uint32; [7] unused.
#include "common.h"
#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int NORM_BLOCKS = 256 * 16;   // the most partial sums a norm leaves: the grid of the other streaming kernels (ew_grid)
constexpr int HYPER_LR = MRCNN_HYPER_LR, HYPER_A = MRCNN_HYPER_A, HYPER_THRESHOLD = MRCNN_HYPER_THRESHOLD, HYPER_SCALE = MRCNN_HYPER_SCALE,
              HYPER_NORM = MRCNN_HYPER_NORM, HYPER_RATE = MRCNN_HYPER_RATE, HYPER_SKIPPED = MRCNN_HYPER_SKIPPED;

inline int ew_grid(size_t n4) { return (int)std::min<size_t>((n4 + NT - 1) / NT, 256 * 16); }
inline int norm_grid(size_t n) { return (int)std::min<size_t>((std::max<size_t>(n / 4, 1) + NT - 1) / NT, NORM_BLOCKS); }

__device__ __forceinline__ bool is_frozen(const uint32_t *__restrict__ frozen, size_t elem) {
    if (frozen == nullptr) return false;
    const size_t blk = elem >> 6;
    return (frozen[blk >> 5] >> (blk & 31)) & 1u;
}

// The section's geometry: `head` single elements, n4 float4 groups, then the tail.
struct Section { size_t head, n4; };
__device__ __forceinline__ Section section_of(size_t n, size_t offset) {
    const size_t lead = (4 - (offset & 3)) & 3, head = lead < n ? lead : n;
    return Section{head, (n - head) / 4};
}
// The single element thread t (< 8) of block 0 owns: one of the 4 possible head elements or of the 4 possible tail elements.
__device__ __forceinline__ bool edge_element(const Section s, size_t n, size_t &e) {
    const size_t tail0 = s.head + s.n4 * 4;
    e = threadIdx.x < 4 ? (size_t)threadIdx.x : tail0 + (threadIdx.x - 4);
    return threadIdx.x < 4 ? (size_t)threadIdx.x < s.head : e < n;
}

template <bool FIRST>
__global__ __launch_bounds__(NT) void k_accumulate(float *__restrict__ acc, const float *__restrict__ g, size_t n, size_t offset,
                                                   const uint32_t *__restrict__ frozen) {
    const Section s = section_of(n, offset);
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < s.n4; i += (size_t)gridDim.x * NT) {
        const size_t e = s.head + i * 4;
        if (is_frozen(frozen, offset + e)) continue;
        float4 gg = ld4(g + e);
        if (!FIRST) {
            const float4 aa = ld4(acc + e);
            gg.x = aa.x + gg.x; gg.y = aa.y + gg.y; gg.z = aa.z + gg.z; gg.w = aa.w + gg.w;
        }
        st4(acc + e, gg);
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        size_t e;
        if (edge_element(s, n, e) && !is_frozen(frozen, offset + e)) acc[e] = FIRST ? g[e] : acc[e] + g[e];
    }
}

// Sum over the threads of a block, in a fixed order (a tree over LDS); the result is valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

template <bool ACC>
__global__ __launch_bounds__(NT) void k_sqnorm(const float *__restrict__ acc, const float *__restrict__ g, size_t n, size_t offset,
                                               const uint32_t *__restrict__ frozen, double *__restrict__ partial) {
    __shared__ double sh[NT];
    const Section s = section_of(n, offset);
    double sum = 0.0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < s.n4; i += (size_t)gridDim.x * NT) {
        const size_t e = s.head + i * 4;
        if (is_frozen(frozen, offset + e)) continue;
        float4 gg = ld4(g + e);
        if (ACC) {
            const float4 aa = ld4(acc + e);
            gg.x = aa.x + gg.x; gg.y = aa.y + gg.y; gg.z = aa.z + gg.z; gg.w = aa.w + gg.w;
        }
        sum = sum + (double)gg.x * (double)gg.x;
        sum = sum + (double)gg.y * (double)gg.y;
        sum = sum + (double)gg.z * (double)gg.z;
        sum = sum + (double)gg.w * (double)gg.w;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        size_t e;
        if (edge_element(s, n, e) && !is_frozen(frozen, offset + e)) {
            const float ge = ACC ? acc[e] + g[e] : g[e];
            sum = sum + (double)ge * (double)ge;
        }
    }
    const double total = block_sum(sum, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(NT) void k_norm_finish(const double *__restrict__ partial, int nb, float *__restrict__ hyper) {
    __shared__ double sh[NT];
    double sum = 0.0;
    for (int i = threadIdx.x; i < nb; i += NT) sum = sum + partial[i];
    const double S = block_sum(sum, sh);
    if (threadIdx.x == 0) {
        const float a = hyper[HYPER_A], threshold = hyper[HYPER_THRESHOLD];
        const float norm = (float)sqrt(S) * a;
        float rate, scale;
        if (isfinite(norm)) {
            rate = norm > threshold ? threshold / norm : 1.0f;
            scale = a * rate;
        } else {        // one bad batch: the update is skipped (momentum decays, weight decay still acts) and counted
            rate = 0.0f;
            scale = 0.0f;
            hyper[HYPER_SKIPPED] = __uint_as_float(__float_as_uint(hyper[HYPER_SKIPPED]) + 1u);     // (a uint32 kept in a float slot: bits only)
        }
        hyper[HYPER_NORM] = norm;
        hyper[HYPER_RATE] = rate;
        hyper[HYPER_SCALE] = scale;
    }
}

// gs = ge * scale with scale == 0 must be 0 for a non-finite ge as well (inf * 0 = nan): a skipped update takes gs = 0.
__device__ __forceinline__ float scaled(float ge, float scale) { return scale == 0.0f ? 0.0f : ge * scale; }

template <bool ACC>
__global__ __launch_bounds__(NT) void k_sgd_hyper(float *__restrict__ p, const float *__restrict__ acc, const float *__restrict__ g,
                                                  float *__restrict__ v, size_t n, size_t offset, const uint32_t *__restrict__ frozen,
                                                  const float *__restrict__ hyper, float momentum, float wd) {
    const float lr = hyper[HYPER_LR], scale = hyper[HYPER_SCALE];
    const Section s = section_of(n, offset);
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < s.n4; i += (size_t)gridDim.x * NT) {
        const size_t e = s.head + i * 4;
        if (is_frozen(frozen, offset + e)) continue;
        float4 pp = ld4(p + e), vv = ld4(v + e);
        float4 gg = ld4(g + e);
        if (ACC) {
            const float4 aa = ld4(acc + e);
            gg.x = aa.x + gg.x; gg.y = aa.y + gg.y; gg.z = aa.z + gg.z; gg.w = aa.w + gg.w;
        }
        gg.x = scaled(gg.x, scale); gg.y = scaled(gg.y, scale); gg.z = scaled(gg.z, scale); gg.w = scaled(gg.w, scale);
        vv.x = momentum * vv.x - lr * (gg.x + wd * pp.x); vv.y = momentum * vv.y - lr * (gg.y + wd * pp.y);
        vv.z = momentum * vv.z - lr * (gg.z + wd * pp.z); vv.w = momentum * vv.w - lr * (gg.w + wd * pp.w);
        pp.x += vv.x; pp.y += vv.y; pp.z += vv.z; pp.w += vv.w;
        st4(p + e, pp);
        st4(v + e, vv);
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        size_t e;
        if (edge_element(s, n, e) && !is_frozen(frozen, offset + e)) {
            const float gs = scaled(ACC ? acc[e] + g[e] : g[e], scale);
            const float nv = momentum * v[e] - lr * (gs + wd * p[e]);
            v[e] = nv;
            p[e] += nv;
        }
    }
}

int chk(bool ok, const char *what) { return ok ? 0 : mrcnn::fail_arg(MRCNN_E_INVALID, "%s", what); }

// What every entry point asks of a section: it lies inside the mask (when there is one) and its pointers are element `offset` of
// 16-byte aligned flat buffers.
int chk_section(const char *name, size_t n, size_t offset, const uint32_t *frozen, size_t n_blocks, const void *a, const void *b,
                const void *c, const void *d) {
    if (offset + n < n) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: offset + n overflows", name);
    if (frozen && (offset + n + 63) / 64 > n_blocks)
        return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: [offset, offset + n) lies outside the n_blocks x 64 floats the mask covers", name);
    const uintptr_t want = (offset & 3) * sizeof(float);
    for (const void *q : {a, b, c, d})
        if (q && ((uintptr_t)q & 15) != want)
            return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: the buffers must be element `offset` of 16-byte aligned flat buffers", name);
    if ((uintptr_t)frozen & 3) return mrcnn::fail_arg(MRCNN_E_INVALID, "%s: the mask must be 4-byte aligned", name);
    return 0;
}

}  // namespace

extern "C" int mrcnn_grad_accumulate_f32(float *acc, const float *g, size_t n, size_t offset, const uint32_t *frozen_blocks,
                                         size_t n_blocks, int first, void *stream) {
    if (n == 0) return 0;
    if (int e = chk(acc && g, "grad_accumulate: null pointer")) return e;
    if (int e = chk(acc != g, "grad_accumulate: acc and g must be different buffers")) return e;
    if (int e = chk_section("grad_accumulate", n, offset, frozen_blocks, n_blocks, acc, g, nullptr, nullptr)) return e;
    const dim3 grid(ew_grid(std::max<size_t>(n / 4, 1))), block(NT);
    if (first) hipLaunchKernelGGL(k_accumulate<true>, grid, block, 0, (hipStream_t)stream, acc, g, n, offset, frozen_blocks);
    else hipLaunchKernelGGL(k_accumulate<false>, grid, block, 0, (hipStream_t)stream, acc, g, n, offset, frozen_blocks);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mrcnn_grad_norm_workspace_bytes(size_t n) { return (size_t)norm_grid(n) * sizeof(double); }

extern "C" int mrcnn_grad_norm_hyper_f32(const float *acc, const float *g, size_t n, size_t offset, const uint32_t *frozen_blocks,
                                         size_t n_blocks, float *hyper, void *workspace, size_t workspace_bytes, void *stream) {
    if (int e = chk(g && hyper && workspace, "grad_norm_hyper: null pointer")) return e;
    if (int e = chk(n > 0, "grad_norm_hyper: n must be positive")) return e;
    if (int e = chk_section("grad_norm_hyper", n, offset, frozen_blocks, n_blocks, acc, g, nullptr, nullptr)) return e;
    if (int e = chk(((uintptr_t)hyper & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
                    "grad_norm_hyper: the hyper block must be 4-byte, the workspace 8-byte aligned")) return e;
    const int nb = norm_grid(n);
    if (int e = chk(workspace_bytes >= (size_t)nb * sizeof(double), "grad_norm_hyper: workspace too small (mrcnn_grad_norm_workspace_bytes)")) return e;
    double *partial = static_cast<double *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (acc) hipLaunchKernelGGL(k_sqnorm<true>, dim3(nb), dim3(NT), 0, st, acc, g, n, offset, frozen_blocks, partial);
    else hipLaunchKernelGGL(k_sqnorm<false>, dim3(nb), dim3(NT), 0, st, acc, g, n, offset, frozen_blocks, partial);
    MRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_norm_finish, dim3(1), dim3(NT), 0, st, partial, nb, hyper);
    MRCNN_LAUNCH_CHECK();
    return 0;
}

extern "C" int mrcnn_sgd_momentum_wd_hyper_f32(float *p, const float *acc, const float *g, float *v, size_t n, size_t offset,
                                               const uint32_t *frozen_blocks, size_t n_blocks, const float *hyper, float momentum,
                                               float weight_decay, void *stream) {
    if (n == 0) return 0;
    if (int e = chk(p && g && v && hyper, "sgd_momentum_wd_hyper: null pointer")) return e;
    if (int e = chk_section("sgd_momentum_wd_hyper", n, offset, frozen_blocks, n_blocks, p, acc, g, v)) return e;
    if (int e = chk(((uintptr_t)hyper & 3) == 0, "sgd_momentum_wd_hyper: the hyper block must be 4-byte aligned")) return e;
    const dim3 grid(ew_grid(std::max<size_t>(n / 4, 1))), block(NT);
    hipStream_t st = (hipStream_t)stream;
    if (acc) hipLaunchKernelGGL(k_sgd_hyper<true>, grid, block, 0, st, p, acc, g, v, n, offset, frozen_blocks, hyper, momentum, weight_decay);
    else hipLaunchKernelGGL(k_sgd_hyper<false>, grid, block, 0, st, p, acc, g, v, n, offset, frozen_blocks, hyper, momentum, weight_decay);
    MRCNN_LAUNCH_CHECK();
    return 0;
}
