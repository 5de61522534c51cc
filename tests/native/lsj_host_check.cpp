// Host-side check of the large-scale-jitter entry points (csrc/augment.hip), a stand-alone program meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer WITHOUT a GPU: compiled together with augment.hip and lib.hip (host code sanitized,
// device code as usual) by tests/test_lsj_cpu.py::test_crop_argument_checks_under_host_sanitizers.
// Every call carries exactly one bad argument and must return MRCNN_E_INVALID with a message before anything is launched: the checks
// read the host descriptor table and compare sizes - they never dereference a device pointer, overflow or divide by zero.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "mrcnn_hip.h"

static int failures = 0;
#define EXPECT_INVALID(call)                                                                                                  \
    do {                                                                                                                      \
        const int rc_ = (call);                                                                                               \
        if (rc_ != MRCNN_E_INVALID) { std::printf("FAIL %s:%d: %s returned %d\n", __FILE__, __LINE__, #call, rc_); ++failures; } \
        else if (std::strlen(mrcnn_last_error()) == 0) { std::printf("FAIL %s:%d: no message\n", __FILE__, __LINE__); ++failures; } \
    } while (0)

static unsigned char *const SRC = reinterpret_cast<unsigned char *>(uintptr_t(4096));     // aligned non-null addresses, never dereferenced
static void *const A16 = reinterpret_cast<void *>(uintptr_t(8192));
static void *const ODD = reinterpret_cast<void *>(uintptr_t(8196));
static const size_t BYTES = 1000000;

static int image(const mrcnn_crop_desc_t *d, int N = 1, int h = 8, int w = 8, void *dst = A16, const unsigned char *src = SRC, size_t bytes = BYTES) {
    return mrcnn_image_resize_crop_batch_u8_f32(src, bytes, d, N, (float *)dst, h, w, 255.0f, nullptr);
}
static int boxes(const mrcnn_crop_desc_t *d, int N = 1, int h = 8, int w = 8, int Gin = 2, int G = 2, void *labels_in = A16, void *bboxes = A16,
                 void *labels = A16, void *gather = A16, void *ws = A16, const unsigned char *src = SRC, size_t bytes = BYTES) {
    return mrcnn_mask_crop_boxes_u8(src, bytes, d, N, Gin, G, h, w, (const int32_t *)labels_in, (float *)bboxes, (int32_t *)labels,
                                    (int32_t *)gather, (int32_t *)ws, nullptr);
}
static int masks(const mrcnn_crop_desc_t *d, int N = 1, int h = 8, int w = 8, int G = 2, void *gather = A16, void *dst = A16,
                 const unsigned char *src = SRC, size_t bytes = BYTES) {
    return mrcnn_mask_resize_crop_batch_nearest_u8(src, bytes, d, N, G, (const int32_t *)gather, (unsigned char *)dst, h, w, nullptr);
}

int main() {
    static_assert(sizeof(mrcnn_crop_desc_t) == 48, "mrcnn_crop_desc_t is 48 bytes");
    // a good descriptor for an 8 x 8 canvas: a 4 x 6 source resized virtually to 16 x 12, the 8 x 8 window at (3, 2)
    const mrcnn_crop_desc_t good_m = {0, 4, 6, 16, 12, 0, 1, 3, 2, 8, 8};
    mrcnn_crop_desc_t good_i = good_m;
    good_i.count = 0;                                       // (images carry no count)
    std::vector<mrcnn_crop_desc_t> bad;
    auto with = [&](auto set) { mrcnn_crop_desc_t d = good_m; set(d); bad.push_back(d); };
    with([](mrcnn_crop_desc_t &d) { d.ch = 9; });           // ch > dst_h
    with([](mrcnn_crop_desc_t &d) { d.cw = 9; });           // cw > dst_w
    with([](mrcnn_crop_desc_t &d) { d.y0 = 9; });           // y0 + ch > oh
    with([](mrcnn_crop_desc_t &d) { d.x0 = 5; });           // x0 + cw > ow
    with([](mrcnn_crop_desc_t &d) { d.y0 = -1; });
    with([](mrcnn_crop_desc_t &d) { d.x0 = -1; });
    with([](mrcnn_crop_desc_t &d) { d.y0 = INT_MIN; });     // oh - y0 must not overflow
    with([](mrcnn_crop_desc_t &d) { d.x0 = INT_MAX; });
    with([](mrcnn_crop_desc_t &d) { d.ch = 0; });
    with([](mrcnn_crop_desc_t &d) { d.cw = -3; });
    with([](mrcnn_crop_desc_t &d) { d.ch = INT_MAX; });
    with([](mrcnn_crop_desc_t &d) { d.H = 0; });
    with([](mrcnn_crop_desc_t &d) { d.W = -6; });
    with([](mrcnn_crop_desc_t &d) { d.oh = 0; });
    with([](mrcnn_crop_desc_t &d) { d.ow = INT_MIN; });
    with([](mrcnn_crop_desc_t &d) { d.flip = 2; });
    with([](mrcnn_crop_desc_t &d) { d.src_offset = -1; });
    with([](mrcnn_crop_desc_t &d) { d.src_offset = (long long)BYTES - 23; });      // a 4 x 6 mask reads 24 bytes, the image 72
    with([](mrcnn_crop_desc_t &d) { d.src_offset = LLONG_MAX; });
    for (mrcnn_crop_desc_t d : bad) {
        EXPECT_INVALID(boxes(&d));
        EXPECT_INVALID(masks(&d));
        d.count = 0;
        EXPECT_INVALID(image(&d));
    }
    // sizes and pointers every entry point checks
    const int Ns[] = {0, -1, MRCNN_RESIZE_BATCH_MAX + 1, INT_MAX};
    for (int N : Ns) {
        EXPECT_INVALID(image(&good_i, N));
        EXPECT_INVALID(boxes(&good_m, N));
        EXPECT_INVALID(masks(&good_m, N));
    }
    const int hw[][2] = {{0, 8}, {8, 0}, {-8, 8}, {INT_MAX, INT_MAX}, {65536, 65536}};
    for (const auto &s : hw) {
        EXPECT_INVALID(image(&good_i, 1, s[0], s[1]));
        EXPECT_INVALID(boxes(&good_m, 1, s[0], s[1]));
        EXPECT_INVALID(masks(&good_m, 1, s[0], s[1]));
    }
    EXPECT_INVALID(image(nullptr));
    EXPECT_INVALID(boxes(nullptr));
    EXPECT_INVALID(masks(nullptr));
    EXPECT_INVALID(image(&good_i, 1, 8, 8, nullptr));
    EXPECT_INVALID(image(&good_i, 1, 8, 8, ODD));
    EXPECT_INVALID(image(&good_i, 1, 8, 8, A16, nullptr));
    EXPECT_INVALID(image(&good_i, 1, 8, 8, A16, SRC, 71));
    EXPECT_INVALID(masks(&good_m, 1, 8, 8, 2, nullptr));                    // a null gather table
    EXPECT_INVALID(masks(&good_m, 1, 8, 8, 2, A16, nullptr));
    EXPECT_INVALID(masks(&good_m, 1, 8, 8, 2, A16, ODD));
    EXPECT_INVALID(masks(&good_m, 1, 8, 8, 2, A16, A16, nullptr));
    EXPECT_INVALID(masks(&good_m, 1, 8, 8, 2, A16, A16, SRC, 23));
    EXPECT_INVALID(masks(&good_m, 1, 8, 8, 0));
    EXPECT_INVALID(masks(&good_m, 1, 8, 8, 65536));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 0, 2));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 0));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 65536, 2));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, INT_MIN));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, nullptr));                 // labels_in, bboxes, labels, gather, ws
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, nullptr));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, ODD));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, A16, nullptr));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, A16, A16, nullptr));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, A16, A16, A16, nullptr));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, A16, A16, A16, ODD));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, A16, A16, A16, A16, nullptr));
    EXPECT_INVALID(boxes(&good_m, 1, 8, 8, 2, 2, A16, A16, A16, A16, A16, SRC, 23));
    mrcnn_crop_desc_t many = good_m;
    many.count = 3;                                         // count > Gin; negative; a count whose bytes overflow 32 bits
    EXPECT_INVALID(boxes(&many));
    many.count = -1;
    EXPECT_INVALID(boxes(&many));
    EXPECT_INVALID(masks(&many));
    many = good_m;
    many.H = many.W = 46341;
    many.count = 65535;
    EXPECT_INVALID(boxes(&many, 1, 8, 8, 65535));
    EXPECT_INVALID(masks(&many, 1, 8, 8, 65535));
    // the second descriptor of a table is checked too, and the table is read only up to N
    mrcnn_crop_desc_t two[2] = {good_m, bad[0]};
    EXPECT_INVALID(boxes(two, 2));
    EXPECT_INVALID(masks(two, 2));
    std::printf(failures ? "lsj_host_check: %d FAILURES\n" : "lsj_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
