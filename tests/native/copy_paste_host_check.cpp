// Host-side check of the Copy-Paste entry points (csrc/copy_paste.hip), a stand-alone program meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer WITHOUT a GPU: compiled together with copy_paste.hip and lib.hip (host code sanitized,
// device code as usual) by tests/test_copy_paste_cpu.py::test_copy_paste_argument_checks_under_host_sanitizers.
// Every call carries exactly one bad argument and must return MRCNN_E_INVALID with a message before anything is launched: the checks
// compare pointers and sizes - they never dereference a device pointer, overflow or divide by zero.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "mrcnn_hip.h"

static int failures = 0;
#define EXPECT_INVALID(call)                                                                                                  \
    do {                                                                                                                      \
        const int rc_ = (call);                                                                                               \
        if (rc_ != MRCNN_E_INVALID) { std::printf("FAIL %s:%d: %s returned %d\n", __FILE__, __LINE__, #call, rc_); ++failures; } \
        else if (std::strlen(mrcnn_last_error()) == 0) { std::printf("FAIL %s:%d: no message\n", __FILE__, __LINE__); ++failures; } \
    } while (0)

static void *const A16 = reinterpret_cast<void *>(uintptr_t(8192));       // an aligned non-null address, never dereferenced
static void *const ODD = reinterpret_cast<void *>(uintptr_t(8196));

struct Sizes {
    int N = 2, G = 3, Gin = 3, G_out = 4, H = 8, W = 8;
};

// q[0..5] = imgs, masks, labels, gather, sel, receive; q[6..7] = out_imgs, alpha
static int image(const Sizes &s, void *const (&q)[8]) {
    return mrcnn_copy_paste_image_f32((const float *)q[0], (const unsigned char *)q[1], (const int32_t *)q[2], (const int32_t *)q[3],
                                      (const unsigned char *)q[4], (const unsigned char *)q[5], s.N, s.G, s.Gin, s.H, s.W, (float *)q[6],
                                      (unsigned char *)q[7], nullptr);
}
// q[0..5] = masks, alpha, labels, gather, sel, receive; q[6..10] = out_masks, bboxes, labels_out, source, ws
static int masks(const Sizes &s, void *const (&q)[11]) {
    return mrcnn_copy_paste_masks_u8((const unsigned char *)q[0], (const unsigned char *)q[1], (const int32_t *)q[2], (const int32_t *)q[3],
                                     (const unsigned char *)q[4], (const unsigned char *)q[5], s.N, s.G, s.Gin, s.G_out, s.H, s.W,
                                     (unsigned char *)q[6], (float *)q[7], (int32_t *)q[8], (int32_t *)q[9], (int32_t *)q[10], nullptr);
}

int main() {
    const Sizes good;
    void *gi[8], *gm[11];
    for (void *&p : gi) p = A16;
    for (void *&p : gm) p = A16;
    // every pointer, NULL in turn; the outputs and the workspace that take 16-byte accesses, misaligned in turn
    for (int k = 0; k < 8; ++k) {
        void *q[8];
        std::memcpy(q, gi, sizeof q);
        q[k] = nullptr;
        EXPECT_INVALID(image(good, q));
        if (k >= 6) {
            q[k] = ODD;
            EXPECT_INVALID(image(good, q));
        }
    }
    for (int k = 0; k < 11; ++k) {
        void *q[11];
        std::memcpy(q, gm, sizeof q);
        q[k] = nullptr;
        EXPECT_INVALID(masks(good, q));
        if (k == 6 || k == 7 || k == 10) {
            q[k] = ODD;
            EXPECT_INVALID(masks(good, q));
        }
    }
    // sizes
    auto both = [&](Sizes s) {
        EXPECT_INVALID(image(s, gi));
        EXPECT_INVALID(masks(s, gm));
    };
    const int Ns[] = {1, 0, -1, MRCNN_RESIZE_BATCH_MAX + 1, INT_MAX, INT_MIN};
    for (int v : Ns) { Sizes s; s.N = v; both(s); }
    const int Gs[] = {0, -1, 65536, INT_MAX, INT_MIN};
    for (int v : Gs) {
        Sizes s;
        s.G = v;
        both(s);
        s = Sizes();
        s.Gin = v;
        both(s);
        s = Sizes();
        s.G_out = v;
        EXPECT_INVALID(masks(s, gm));
    }
    const int hw[][2] = {{0, 8}, {8, 0}, {-8, 8}, {8, -8}, {INT_MAX, INT_MAX}, {65536, 65536}, {INT_MAX, 1}, {1, INT_MAX}, {INT_MIN, 8},
                         {8, INT_MIN}, {46341, 46341}};
    for (const auto &d : hw) { Sizes s; s.H = d[0]; s.W = d[1]; both(s); }
    // the largest sizes the checks accept do not overflow on their way there: one bad pointer behind them is still what is refused
    Sizes big;
    big.N = MRCNN_RESIZE_BATCH_MAX; big.G = big.Gin = big.G_out = 65535; big.H = 32768; big.W = 65521;
    void *q[11];
    std::memcpy(q, gm, sizeof q);
    q[10] = nullptr;
    EXPECT_INVALID(masks(big, q));
    void *r[8];
    std::memcpy(r, gi, sizeof r);
    r[7] = ODD;
    EXPECT_INVALID(image(big, r));
    std::printf(failures ? "copy_paste_host_check: %d FAILURES\n" : "copy_paste_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
