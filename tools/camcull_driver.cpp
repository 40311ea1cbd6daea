// DIAGNOSTIC: a stand-alone host program over the tile classifier (csrc/ptmi_camcull.h), for sanitizer
// builds -- no HIP, no Python:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pathtracer-ocl_amd/csrc tools/camcull_driver.cpp -o /tmp/camcull_driver && /tmp/camcull_driver
// The Cornell box of the reference scene (floor / ceiling, left / right, back; two balls and the flattened
// light) seen from (0, 0.1, -1.5) towards +z, at 160 x 120 and 100 x 75 (partial edge tiles), and a camera
// record full of NaN (every bit must stay set).  Prints how many tiles keep how many planes / spheres.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ptmi_camcull.h"

using namespace ptmi;

static DevCamera camera(int w, int h) {
    DevCamera c{};
    c.width = w, c.height = h;
    const double half_view = std::tan(1.0471975511965976 / 2), aspect = (double)w / h;
    c.half_width = aspect >= 1 ? half_view : half_view * aspect;
    c.half_height = aspect >= 1 ? half_view / aspect : half_view;
    c.pixel_size = c.half_width * 2 / w;
    const double inv[16] = {-1, 0, 0, 0, 0, 1, 0, 0.1, 0, 0, -1, -1.5, 0, 0, 0, 1};
    std::memcpy(c.inv, inv, sizeof inv);
    for (int r = 0; r < 4; r++) c.origin[r] = inv[4 * r + 3];
    return c;
}

static int run(const DevCamera& cam, bool expect_cull) {
    const double rows[5][4] = {{0, 1, 0, 0.4}, {0, 1, 0, -0.4}, {1, 0, 0, 0.6}, {1, 0, 0, -0.6}, {0, 0, 1, -0.4}};
    const double balls[3][6] = {{0.12, 0.12, 0.12, -0.35, -0.28, -0.15}, {0.16, 0.16, 0.16, 0, -0.24, -0.30},
                                {0.283, 0.01, 0.283, 0, 0.399, 0}};
    std::vector<PlaneRec> planes(5);
    std::vector<SphereRec> spheres(3);
    std::vector<double> cpl(5), csp(kCamSphere * 3);
    const double* o = cam.origin;
    for (int p = 0; p < 5; p++) {
        std::memcpy(planes[p].row1, rows[p], 32);
        cpl[p] = ((rows[p][0] * o[0] + rows[p][1] * o[1]) + rows[p][2] * o[2]) + rows[p][3];
    }
    for (int q = 0; q < 3; q++) {
        SphereRec& Q = spheres[q];
        Q = SphereRec{};
        Q.m0 = 1 / balls[q][0], Q.m5 = 1 / balls[q][1], Q.m10 = 1 / balls[q][2], Q.m15 = 1;
        Q.m3 = -balls[q][3] * Q.m0, Q.m7 = -balls[q][4] * Q.m5, Q.m11 = -balls[q][5] * Q.m10;
        double* t = &csp[kCamSphere * q];
        t[0] = Q.m0 * o[0] + Q.m3, t[1] = Q.m5 * o[1] + Q.m7, t[2] = Q.m10 * o[2] + Q.m11;
        t[3] = std::fma(t[2], t[2], std::fma(t[1], t[1], t[0] * t[0])) - 1.0;
    }
    const int tx = (cam.width + 7) / 8, ty = (cam.height + 7) / 8;
    int np_hist[6] = {}, ns_hist[4] = {}, culled = 0;
    for (int t = 0; t < tx * ty; t++) {
        const uint32_t m = cull_tile_mask(cam, planes.data(), 5, spheres.data(), 3, cpl.data(), csp.data(), t % tx, t / tx);
        if ((m | 0x0007001Fu) != 0xFFFFFFFFu) return std::printf("tile %d: a bit without an object is cleared\n", t), 1;
        np_hist[__builtin_popcount(m & 0x1F)]++;
        ns_hist[__builtin_popcount((m >> 16) & 7)]++;
        culled += m != 0xFFFFFFFFu;
    }
    std::printf("%dx%d: %d of %d tiles culled; planes kept 0..5: %d %d %d %d %d %d; spheres kept 0..3: %d %d %d %d\n",
                cam.width, cam.height, culled, tx * ty, np_hist[0], np_hist[1], np_hist[2], np_hist[3], np_hist[4],
                np_hist[5], ns_hist[0], ns_hist[1], ns_hist[2], ns_hist[3]);
    return (culled > 0) == expect_cull ? 0 : 1;
}

int main() {
    int rc = run(camera(160, 120), true) | run(camera(100, 75), true);
    DevCamera bad = camera(64, 48);
    for (double& v : bad.inv) v = NAN;
    rc |= run(bad, false);
    std::printf(rc ? "FAILED\n" : "ok\n");
    return rc;
}
