// Host-side check of the active-row entry points (mrcnn_active_rows_u8, mrcnn_conv2d_bwd_data_active_f32,
// mrcnn_conv2d_bwd_filter_active_f32), meant to run under AddressSanitizer WITHOUT a GPU like abi_host_check.cpp
// (make -C chainer-maskrcnn_amd/csrc asan; tests/test_mask_bwd_skip_cpu.py): null buffers, a mask of the wrong length and nonsensical
// sizes must each return a negative code with a message before anything is launched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "mrcnn_hip.h"

static int failures = 0;
#define EXPECT_ERR(call)                                                      \
    do {                                                                      \
        const int rc_ = (call);                                               \
        if (rc_ == 0) { std::printf("FAIL %s:%d: %s returned 0\n", __FILE__, __LINE__, #call); ++failures; } \
        else if (rc_ > 0) { std::printf("FAIL %s:%d: reached the HIP runtime (code %d) instead of rejecting its arguments: %s\n", __FILE__, __LINE__, rc_, #call); ++failures; } \
        else if (std::strlen(mrcnn_last_error()) == 0) { std::printf("FAIL %s:%d: no message\n", __FILE__, __LINE__); ++failures; } \
    } while (0)

int main() {
    static float buf[64];
    static unsigned char act[8];
    static int32_t n_pos[2];
    float *F = nullptr;
    const float *CF = nullptr;
    void *V = nullptr;
    // ---- the mask kernel: sizes first, then pointers; an empty batch is valid and launches nothing
    EXPECT_ERR(mrcnn_active_rows_u8(n_pos, 2, 0, act, V));
    EXPECT_ERR(mrcnn_active_rows_u8(n_pos, -1, 4, act, V));
    EXPECT_ERR(mrcnn_active_rows_u8(n_pos, 1 << 20, 1 << 12, act, V));
    EXPECT_ERR(mrcnn_active_rows_u8(nullptr, 2, 4, act, V));
    EXPECT_ERR(mrcnn_active_rows_u8(n_pos, 2, 4, nullptr, V));
    if (mrcnn_active_rows_u8(nullptr, 0, 4, nullptr, V) != 0) { std::printf("FAIL: an empty batch is valid\n"); ++failures; }
    // ---- the two backward passes: the plain calls' checks hold with and without a mask ...
    EXPECT_ERR(mrcnn_conv2d_bwd_data_active_f32(CF, CF, F, CF, 1, 8, 8, 32, 32, 3, 3, 1, 1, 0, nullptr, 0, V, 0, V));
    EXPECT_ERR(mrcnn_conv2d_bwd_data_active_f32(CF, CF, F, CF, 8, 8, 8, 32, 32, 3, 3, 1, 1, 0, act, 8, V, 0, V));
    EXPECT_ERR(mrcnn_conv2d_bwd_filter_active_f32(CF, CF, F, F, 1, 8, 8, 32, 32, 3, 3, 1, 1, 0, CF, nullptr, 0, V, 0, V));
    EXPECT_ERR(mrcnn_conv2d_bwd_filter_active_f32(CF, CF, F, F, 8, 8, 8, 32, 32, 3, 3, 1, 1, 0, CF, act, 8, V, 0, V));
    EXPECT_ERR(mrcnn_conv2d_bwd_data_active_f32(buf, buf, buf, CF, 8, 8, 8, 32, 32, 3, 3, 2, 1, 0, act, 8, V, 0, V));          /* stride 1 only */
    EXPECT_ERR(mrcnn_conv2d_bwd_filter_active_f32(buf, buf, buf, buf, 8, 14, 14, 256, 256, 3, 3, 1, 1, 0, CF, act, 8, buf, 16, V));   /* short workspace */
    // ... and a mask must have one entry per image
    EXPECT_ERR(mrcnn_conv2d_bwd_data_active_f32(buf, buf, buf, CF, 8, 8, 8, 32, 32, 3, 3, 1, 1, 0, act, 7, V, 0, V));
    EXPECT_ERR(mrcnn_conv2d_bwd_data_active_f32(buf, buf, buf, CF, 8, 8, 8, 32, 32, 3, 3, 1, 1, 0, act, 0, V, 0, V));
    EXPECT_ERR(mrcnn_conv2d_bwd_filter_active_f32(buf, buf, buf, buf, 8, 8, 8, 32, 32, 3, 3, 1, 1, 0, CF, act, 9, buf, sizeof buf, V));
    std::printf("active_rows_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
