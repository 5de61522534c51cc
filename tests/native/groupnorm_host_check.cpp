// Host-side check of the GroupNorm entry points (csrc/groupnorm.hip), a stand-alone program meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer WITHOUT a GPU: compiled together with groupnorm.hip and lib.hip (host code sanitized,
// device code as usual) by tests/test_groupnorm_cpu.py::test_group_norm_argument_checks_under_host_sanitizers.
// The plan query is swept over geometries (host arithmetic only); every compute call carries exactly one bad argument and must return
// MRCNN_E_INVALID with a message before anything is launched: the checks compare pointers and sizes - they never dereference a device
// pointer, overflow or divide by zero.
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
#define EXPECT(cond)                                                                                         \
    do {                                                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; }              \
    } while (0)

static void *const A16 = reinterpret_cast<void *>(uintptr_t(8192));       // an aligned non-null address, never dereferenced
static void *const ODD = reinterpret_cast<void *>(uintptr_t(8196));

struct Sizes {
    int R = 2, H = 7, W = 7, C = 64, Cp = 64, G = 32, relu = 1;
    float eps = 1e-5f;
    size_t ws_bytes = 2 * 2 * 64 * sizeof(float);
};

// q[0..2] = x, gamma, beta; q[3] = y; q[4..5] = mean, rstd (nullable)
static int fwd(const Sizes &s, void *const (&q)[6]) {
    return mrcnn_group_norm_fwd_f32((const float *)q[0], (const float *)q[1], (const float *)q[2], s.R, s.H, s.W, s.C, s.Cp, s.G, s.eps, s.relu,
                                    (float *)q[3], (float *)q[4], (float *)q[5], nullptr);
}
// q[0..5] = gy, x, gamma, beta, mean, rstd; q[6..8] = gx, ggamma, gbeta; q[9] = ws
static int bwd(const Sizes &s, void *const (&q)[10]) {
    return mrcnn_group_norm_bwd_f32((const float *)q[0], (const float *)q[1], (const float *)q[2], (const float *)q[3], (const float *)q[4],
                                    (const float *)q[5], s.R, s.H, s.W, s.C, s.Cp, s.G, s.relu, (float *)q[6], (float *)q[7], (float *)q[8], 0,
                                    q[9], s.ws_bytes, nullptr);
}

int main() {
    const Sizes good;
    void *gf[6], *gb[10];
    for (void *&p : gf) p = A16;
    for (void *&p : gb) p = A16;
    // the plan query: both paths, the workspace size, nullable outputs
    const int Cs[][3] = {{32, 32, 32}, {64, 64, 32}, {256, 256, 32}, {96, 96, 32}, {48, 64, 16}, {96, 96, 8}, {512, 512, 8}, {2048, 2048, 2},
                         {7, 8, 7}, {6, 8, 2}, {20, 32, 1}};
    for (const auto &c : Cs)
        for (int hw = 1; hw <= 1100; hw += (hw < 300 ? 1 : 37)) {
            int path = -1;
            size_t nb = 0;
            EXPECT(mrcnn_group_norm_plan(3, 1, hw, c[0], c[1], c[2], &path, &nb) == 0);
            EXPECT(path == 0 || path == 1);
            EXPECT(nb == size_t(2) * 3 * c[1] * sizeof(float));
            const int cpg = c[0] / c[2];
            if (!(cpg == 1 || cpg == 2 || cpg % 4 == 0)) EXPECT(path == 1);
            else if (32 % cpg == 0) EXPECT(path == (hw <= 256 ? 0 : 1));     // 8 columns, 32 rows of 8 pixels
        }
    int path = -1;
    EXPECT(mrcnn_group_norm_plan(512, 14, 14, 256, 256, 32, &path, nullptr) == 0 && path == 0);
    EXPECT(mrcnn_group_norm_plan(512, 7, 7, 256, 256, 32, &path, nullptr) == 0 && path == 0);
    EXPECT(mrcnn_group_norm_plan(2, 5, 3, 96, 96, 32, &path, nullptr) == 0 && path == 1);
    EXPECT(mrcnn_group_norm_plan(2, 33, 31, 64, 64, 32, &path, nullptr) == 0 && path == 1);
    EXPECT(mrcnn_group_norm_plan(0, 7, 7, 64, 64, 32, nullptr, nullptr) == 0);
    EXPECT(mrcnn_group_norm_plan(INT_MAX, 1, 1, 4, 4, 1, &path, nullptr) == 0);
    // R == 0 succeeds without a launch, whatever the buffers
    {
        Sizes s;
        s.R = 0;
        void *n6[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        void *n10[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        s.ws_bytes = 0;
        EXPECT(fwd(s, n6) == 0);
        EXPECT(bwd(s, n10) == 0);
    }
    // every required pointer, NULL in turn; the ones that take 16-byte accesses, misaligned in turn
    for (int k = 0; k < 4; ++k) {
        void *q[6];
        std::memcpy(q, gf, sizeof q);
        q[k] = nullptr;
        EXPECT_INVALID(fwd(good, q));
        q[k] = ODD;
        EXPECT_INVALID(fwd(good, q));
    }
    for (int k = 0; k < 10; ++k) {
        void *q[10];
        std::memcpy(q, gb, sizeof q);
        q[k] = nullptr;
        EXPECT_INVALID(bwd(good, q));
        if (k != 4 && k != 5) {
            q[k] = ODD;
            EXPECT_INVALID(bwd(good, q));
        }
    }
    // a short workspace
    const size_t shorts[] = {0, 1, good.ws_bytes - 1};
    for (size_t nb : shorts) {
        Sizes s;
        s.ws_bytes = nb;
        EXPECT_INVALID(bwd(s, gb));
    }
    // geometry: each invalid case through all three entry points
    auto all = [&](Sizes s) {
        s.ws_bytes = SIZE_MAX;
        EXPECT_INVALID(mrcnn_group_norm_plan(s.R, s.H, s.W, s.C, s.Cp, s.G, nullptr, nullptr));
        EXPECT_INVALID(fwd(s, gf));
        EXPECT_INVALID(bwd(s, gb));
    };
    { Sizes s; s.G = 24; all(s); }                           // G does not divide C
    { Sizes s; s.G = 128; all(s); }
    { Sizes s; s.Cp = 32; all(s); }                          // Cp < C
    { Sizes s; s.Cp = 66; all(s); }                          // Cp % 4 != 0
    { Sizes s; s.C = 62; s.Cp = 62; s.G = 31; all(s); }
    const int bad[] = {0, -1, INT_MIN};
    for (int v : bad) {
        { Sizes s; s.H = v; all(s); }
        { Sizes s; s.W = v; all(s); }
        { Sizes s; s.C = v; all(s); }
        { Sizes s; s.G = v; all(s); }
        { Sizes s; s.Cp = v; all(s); }
        if (v < 0) { Sizes s; s.R = v; all(s); }
    }
    { Sizes s; s.H = INT_MAX; s.W = INT_MAX; all(s); }       // H * W * Cp beyond int32
    { Sizes s; s.H = 46341; s.W = 46341; all(s); }
    { Sizes s; s.H = 65536; s.W = 512; all(s); }
    { Sizes s; s.R = INT_MAX; all(s); }                      // more workgroups than a grid takes
    { Sizes s; s.relu = 2; EXPECT_INVALID(fwd(s, gf)); EXPECT_INVALID(bwd(s, gb)); }
    { Sizes s; s.relu = -1; EXPECT_INVALID(fwd(s, gf)); EXPECT_INVALID(bwd(s, gb)); }
    { Sizes s; s.eps = 0.f; EXPECT_INVALID(fwd(s, gf)); }
    { Sizes s; s.eps = -1.f; EXPECT_INVALID(fwd(s, gf)); }
    std::printf(failures ? "groupnorm_host_check: %d FAILURES\n" : "groupnorm_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
