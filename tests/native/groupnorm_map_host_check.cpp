// Host-side check of the map GroupNorm entry points (csrc/groupnorm_map.hip), a stand-alone program meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer WITHOUT a GPU: compiled together with groupnorm_map.hip and lib.hip (host code
// sanitized, device code as usual) by tests/test_fpn_groupnorm_cpu.py::test_map_argument_checks_under_host_sanitizers.
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
    int R = 2, H = 40, W = 40, C = 64, Cp = 64, G = 16;
    float eps = 1e-5f;
    size_t ws_bytes = SIZE_MAX;
};

// q[0..2] = x, gamma, beta; q[3] = y; q[4] = ws; q[5..6] = mean, rstd (nullable)
static int fwd(const Sizes &s, void *const (&q)[7]) {
    return mrcnn_group_norm_map_fwd_f32((const float *)q[0], (const float *)q[1], (const float *)q[2], s.R, s.H, s.W, s.C, s.Cp, s.G, s.eps,
                                        (float *)q[3], (float *)q[5], (float *)q[6], q[4], s.ws_bytes, nullptr);
}
// q[0..4] = gy, x, gamma, mean, rstd; q[5..7] = gx, ggamma, gbeta; q[8] = ws
static int bwd(const Sizes &s, void *const (&q)[9]) {
    return mrcnn_group_norm_map_bwd_f32((const float *)q[0], (const float *)q[1], (const float *)q[2], (const float *)q[3], (const float *)q[4],
                                        s.R, s.H, s.W, s.C, s.Cp, s.G, (float *)q[5], (float *)q[6], (float *)q[7], 0, q[8], s.ws_bytes, nullptr);
}

int main() {
    const Sizes good;
    void *gf[7], *gb[9];
    for (void *&p : gf) p = A16;
    for (void *&p : gb) p = A16;
    // the plan query: the chunks cover the map exactly, do not depend on R, and the workspaces are what the header states
    const int Cs[][3] = {{32, 32, 8}, {64, 64, 16}, {256, 256, 32}, {48, 64, 12}, {128, 128, 2}, {256, 256, 1}, {1024, 1024, 4}, {4, 4, 1},
                         {96, 96, 8}, {8, 12, 2}};
    for (const auto &c : Cs)
        for (long long hw = 1; hw <= 3000000; hw = hw < 600 ? hw + 1 : hw * 3 + 7) {
            if (hw * c[1] > INT_MAX) break;
            int ppc = -1, chunks = -1, ppc1 = -1, chunks1 = -1;
            size_t nf = 0, nb = 0, nf1 = 0, nb1 = 0;
            EXPECT(mrcnn_group_norm_map_plan(3, 1, (int)hw, c[0], c[1], c[2], &ppc, &chunks, &nf, &nb) == 0);
            EXPECT(ppc > 0 && chunks > 0);
            EXPECT((long long)chunks * ppc >= hw && hw > (long long)(chunks - 1) * ppc);
            EXPECT(nf == (size_t(2) * 3 * chunks * c[2] + size_t(2) * 3 * c[2]) * sizeof(float));
            EXPECT(nb == (size_t(2) * 3 * chunks * c[1] + size_t(2) * 3 * c[2]) * sizeof(float));
            EXPECT(mrcnn_group_norm_map_plan(7, (int)hw, 1, c[0], c[1], c[2], &ppc1, &chunks1, &nf1, &nb1) == 0);
            EXPECT(ppc1 == ppc && chunks1 == chunks && nf1 >= nf && nb1 >= nb);
        }
    int chunks = -1;
    EXPECT(mrcnn_group_norm_map_plan(2, 256, 256, 256, 256, 32, nullptr, &chunks, nullptr, nullptr) == 0 && 2 * chunks >= 512);
    EXPECT(mrcnn_group_norm_map_plan(2, 32, 32, 256, 256, 32, nullptr, &chunks, nullptr, nullptr) == 0 && chunks >= 16);
    EXPECT(mrcnn_group_norm_map_plan(0, 7, 7, 64, 64, 16, nullptr, nullptr, nullptr, nullptr) == 0);
    EXPECT(mrcnn_group_norm_map_plan(INT_MAX, 1, 1, 4, 4, 1, nullptr, nullptr, nullptr, nullptr) == 0);
    // R == 0 succeeds without a launch, whatever the buffers
    {
        Sizes s;
        s.R = 0;
        s.ws_bytes = 0;
        void *n7[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        void *n9[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        EXPECT(fwd(s, n7) == 0);
        EXPECT(bwd(s, n9) == 0);
    }
    // every required pointer, NULL in turn; the ones that take 16-byte accesses, misaligned in turn
    for (int k = 0; k < 5; ++k) {
        void *q[7];
        std::memcpy(q, gf, sizeof q);
        q[k] = nullptr;
        EXPECT_INVALID(fwd(good, q));
        q[k] = ODD;
        EXPECT_INVALID(fwd(good, q));
    }
    for (int k = 0; k < 9; ++k) {
        void *q[9];
        std::memcpy(q, gb, sizeof q);
        q[k] = nullptr;
        EXPECT_INVALID(bwd(good, q));
        if (k != 3 && k != 4) {
            q[k] = ODD;
            EXPECT_INVALID(bwd(good, q));
        }
    }
    // a short workspace
    {
        size_t nf = 0, nb = 0;
        EXPECT(mrcnn_group_norm_map_plan(good.R, good.H, good.W, good.C, good.Cp, good.G, nullptr, nullptr, &nf, &nb) == 0 && nf > 0 && nb > 0);
        const size_t cut[] = {0, 1, 2};
        for (size_t c : cut) {
            Sizes s;
            s.ws_bytes = c == 2 ? nf - 1 : c;
            EXPECT_INVALID(fwd(s, gf));
            s.ws_bytes = c == 2 ? nb - 1 : c;
            EXPECT_INVALID(bwd(s, gb));
        }
    }
    // geometry: each invalid case through all three entry points
    auto all = [&](const Sizes &s) {
        EXPECT_INVALID(mrcnn_group_norm_map_plan(s.R, s.H, s.W, s.C, s.Cp, s.G, nullptr, nullptr, nullptr, nullptr));
        EXPECT_INVALID(fwd(s, gf));
        EXPECT_INVALID(bwd(s, gb));
    };
    { Sizes s; s.G = 24; all(s); }                           // G does not divide C
    { Sizes s; s.G = 128; all(s); }
    { Sizes s; s.Cp = 32; all(s); }                          // Cp < C
    { Sizes s; s.Cp = 66; all(s); }                          // Cp % 4 != 0
    { Sizes s; s.G = 64; all(s); }                           // cpg 1
    { Sizes s; s.G = 32; all(s); }                           // cpg 2
    { Sizes s; s.C = 48; s.G = 16; all(s); }                 // cpg 3
    { Sizes s; s.C = 96; s.Cp = 96; s.G = 16; all(s); }      // cpg 6
    { Sizes s; s.C = 512; s.Cp = 512; s.G = 1; all(s); }     // cpg above 256
    { Sizes s; s.C = 2048; s.Cp = 2048; s.G = 32; all(s); }  // Cp above 1024
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
    { Sizes s; s.eps = 0.f; EXPECT_INVALID(fwd(s, gf)); }
    { Sizes s; s.eps = -1.f; EXPECT_INVALID(fwd(s, gf)); }
    std::printf(failures ? "groupnorm_map_host_check: %d FAILURES\n" : "groupnorm_map_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
