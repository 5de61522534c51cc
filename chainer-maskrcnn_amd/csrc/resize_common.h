// Source taps of the training Transform's two resizes (OpenCV's coordinate rules, restated exactly as in
// chainer_maskrcnn/dataset/transforms.py), shared by the per-image kernels of nn.hip and the batched kernels of augment.hip so the
// two can never drift apart.  Bit-identical to the host: same float operations, no contraction (-ffp-contract=off).
//   INTER_LINEAR  fx = (float)((dx + 0.5) * (src/dst) - 0.5), sx = floor(fx), clamped taps; horizontal then vertical
//   INTER_NEAREST sx = min(floor(dx * (src/dst)), src - 1)
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void linear_tap(int d, int dst, int src, int &s0, int &s1, float &a0, float &a1) {
    const double scale = 1.0 / ((double)dst / (double)src);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    s0 = s; s1 = min(s + 1, src - 1);
    a0 = 1.0f - f; a1 = f;
}

__device__ __forceinline__ int nearest_tap(int d, int dst, int src) {
    return min((int)floor((double)d * (1.0 / ((double)dst / (double)src))), src - 1);
}
