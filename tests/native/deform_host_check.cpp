// Stand-alone host check of the deformable-convolution corner function (csrc/deform_common.h): the position guard compares in float
// before anything becomes an integer, so a huge or non-finite position must give valid == 0 and indices 0 - and no conversion the
// float-cast-overflow sanitizer objects to.  Built by tests/test_deform_cpu.py with -fsanitize=address,undefined,float-cast-overflow on the
// host code and run on the CPU; no device is touched.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "deform_common.h"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static bool is_nothing(const DeformCorners &t) {
    return t.valid == 0u && t.y0 == 0 && t.x0 == 0 && t.ly == 0.f && t.lx == 0.f && t.hy == 0.f && t.hx == 0.f;
}

// every cell a valid bit names lies inside the map: what the kernels index with
static void check_inside(const DeformCorners &t, int H, int W) {
    for (int c = 0; c < 4; ++c)
        if ((t.valid >> c) & 1u) {
            const int y = t.y0 + (c >> 1), x = t.x0 + (c & 1);
            EXPECT(y >= 0 && y < H && x >= 0 && x < W);
        }
    float sum = 0.f;
    for (int c = 0; c < 4; ++c) {
        const float w = deform_weight(t, c);
        EXPECT(w >= 0.f && w <= 1.f);
        sum += w;
    }
    if (t.valid) EXPECT(std::fabs(sum - 1.f) < 1e-6f);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int shapes[][2] = {{1, 1}, {5, 7}, {6, 5}, {128, 128}, {100, 168}, {1 << 20, 3}};
    for (const auto &hw : shapes) {
        const int H = hw[0], W = hw[1];
        // positions that sample nothing, on either axis and on both
        const float out[] = {1e30f, -1e30f, inf, -inf, nan, -1.0f, (float)H, (float)W, -1.5f, (float)H + 0.25f, (float)W + 7.f, 3e9f, -3e9f,
                             std::numeric_limits<float>::max(), -std::numeric_limits<float>::max()};
        for (float p : out) {
            const bool y_out = !(p > -1.0f && p < (float)H), x_out = !(p > -1.0f && p < (float)W);
            if (y_out) EXPECT(is_nothing(deform_corners(p, 0.5f, H, W)));
            if (x_out) EXPECT(is_nothing(deform_corners(0.5f, p, H, W)));
            if (y_out || x_out) EXPECT(is_nothing(deform_corners(p, p, H, W)));
        }
        EXPECT(is_nothing(deform_corners(-1.0f, 0.f, H, W)) && is_nothing(deform_corners(0.f, -1.0f, H, W)));
        EXPECT(is_nothing(deform_corners((float)H, 0.f, H, W)) && is_nothing(deform_corners(0.f, (float)W, H, W)));
        // the integers in between: weight 1 on the cell itself, the cells beyond it valid only inside the map
        const int ys[] = {0, 1, H / 2, H - 2, H - 1}, xs[] = {0, 1, W / 2, W - 2, W - 1};
        for (int y : ys)
            for (int x : xs) {
                if (y < 0 || x < 0 || y > H - 1 || x > W - 1) continue;
                const DeformCorners t = deform_corners((float)y, (float)x, H, W);
                EXPECT(t.y0 == y && t.x0 == x && t.ly == 0.f && t.lx == 0.f && t.hy == 1.f && t.hx == 1.f);
                EXPECT((t.valid & 1u) && deform_weight(t, 0) == 1.f && deform_weight(t, 1) == 0.f && deform_weight(t, 2) == 0.f &&
                       deform_weight(t, 3) == 0.f);
                EXPECT(((t.valid >> 1) & 1u) == (x + 1 <= W - 1 ? 1u : 0u) && ((t.valid >> 2) & 1u) == (y + 1 <= H - 1 ? 1u : 0u));
                check_inside(t, H, W);
            }
        // just inside the two open ends: only the cells inside the map are valid
        const float lo = std::nextafter(-1.0f, 0.f), hi_y = std::nextafter((float)H, 0.f), hi_x = std::nextafter((float)W, 0.f);
        DeformCorners t = deform_corners(lo, lo, H, W);
        EXPECT(t.y0 == -1 && t.x0 == -1 && t.valid == 8u);
        check_inside(t, H, W);
        t = deform_corners(hi_y, hi_x, H, W);
        EXPECT(t.y0 == H - 1 && t.x0 == W - 1 && t.valid == 1u);
        check_inside(t, H, W);
        // a sweep across the map and its margins, fractional positions included
        for (int i = -12; i <= 4 * 12; ++i)
            for (int j = -12; j <= 4 * 12; ++j) {
                const float py = -2.f + (float)i * ((float)H + 3.f) / 48.f, px = -2.f + (float)j * ((float)W + 3.f) / 48.f;
                const DeformCorners c = deform_corners(py, px, H, W);
                check_inside(c, H, W);
                const bool in = py > -1.f && py < (float)H && px > -1.f && px < (float)W;
                EXPECT(in ? (c.y0 >= -1 && c.y0 <= H - 1 && c.x0 >= -1 && c.x0 <= W - 1) : is_nothing(c));
            }
    }
    // the positions of the taps: tap k = 3 i + j of pixel (y, x) under zero offsets is (y - 1 + i, x - 1 + j); a non-finite offset stays one
    for (int k = 0; k < kDeformTaps; ++k) {
        EXPECT(deform_pos_y(4, k, 0.f) == (float)(3 + k / 3) && deform_pos_x(4, k, 0.f) == (float)(3 + k % 3));
        EXPECT(is_nothing(deform_corners(deform_pos_y(2, k, inf), deform_pos_x(2, k, 0.f), 5, 7)));
        EXPECT(is_nothing(deform_corners(deform_pos_y(2, k, 0.f), deform_pos_x(2, k, nan), 5, 7)));
        EXPECT(is_nothing(deform_corners(deform_pos_y(2, k, -1e30f), deform_pos_x(2, k, 1e30f), 5, 7)));
    }
    if (failures) {
        std::printf("deform_host_check: %d failures\n", failures);
        return 1;
    }
    std::printf("deform_host_check: ok\n");
    return 0;
}
