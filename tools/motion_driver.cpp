// DIAGNOSTIC: a stand-alone host program over the host-only half of object updates (csrc/ptmi_motion.h:
// the identity check of ptmi_scene_set_objects and the motion records of ptmi_motion_table), for
// sanitizer builds -- no HIP, no Python:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pathtracer-ocl_amd/csrc tools/motion_driver.cpp -o /tmp/motion_driver && /tmp/motion_driver
// Records are exactly 1024 bytes on the heap, so a read past one is caught.  Checked: identical records
// are static; a translated sphere's B carries a point of the new surface to the same object-space point
// of the old one and G keeps a normal; a projective record and a NaN give no history; a group's identity
// (type, childCount at its limits, roots, box) is compared without reading past the record.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ptmi_motion.h"

using namespace ptmi;

struct Record {
    std::unique_ptr<uint8_t[]> b{new uint8_t[kObjectBytes]()};
    void mat(int off, const double* m) { std::memcpy(b.get() + off, m, 128); }
    void set(const double* transform, const double* inverse) {
        double it[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) it[4 * r + c] = inverse[4 * c + r];
        mat(0, transform), mat(128, inverse), mat(256, it);
    }
    void type(int64_t t) { std::memcpy(b.get() + 456, &t, 8); }
    void children(int32_t n, int32_t first) {
        std::memcpy(b.get() + 584, &n, 4);
        for (int32_t k = 0; k < n && k < kMaxChildren; k++) {
            const int32_t r = first + k;
            std::memcpy(b.get() + 588 + 4 * k, &r, 4);
        }
    }
    void box(double lo, double hi) {
        const double mn[4] = {lo, lo, lo, 1}, mx[4] = {hi, hi, hi, 1};
        std::memcpy(b.get() + 520, mn, 32), std::memcpy(b.get() + 552, mx, 32);
    }
};

// scale s, then translate (x, y, z), with its exact inverse for s a power of two
static void place(Record& r, double s, double x, double y, double z) {
    const double t[16] = {s, 0, 0, x, 0, s, 0, y, 0, 0, s, z, 0, 0, 0, 1};
    const double i[16] = {1 / s, 0, 0, -x / s, 0, 1 / s, 0, -y / s, 0, 0, 1 / s, -z / s, 0, 0, 0, 1};
    r.set(t, i);
}

static int fail(const char* what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

int main() {
    int rc = 0;
    double m[kMotionDoubles];
    Record a, b;
    a.type(1), b.type(1);
    place(a, 0.125, -0.35, -0.28, -0.15);
    place(b, 0.125, -0.35, -0.28, -0.15);
    motion_record(a.b.get(), b.b.get(), m);
    if (m[21] != 0.0 || m[22] != 0.0 || m[23] != 0.0) rc |= fail("identical records are static");

    place(b, 0.125, -0.25, -0.28, -0.15);  // moved by +0.1 in x
    motion_record(a.b.get(), b.b.get(), m);
    if (m[21] != 1.0) rc |= fail("a translated sphere has moved");
    // the new sphere's surface point above its centre -> the old sphere's
    const double p[3] = {-0.25, -0.28 + 0.125, -0.15}, want[3] = {-0.35, -0.28 + 0.125, -0.15};
    for (int r = 0; r < 3; r++) {
        const double v = ((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3];
        if (std::fabs(v - want[r]) > 1e-15) rc |= fail("B carries the point back");
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            if (m[12 + 3 * r + c] != (r == c ? 1.0 : 0.0)) rc |= fail("G of a translation is the identity");

    double proj[16];
    std::memcpy(proj, b.b.get() + 128, 128);
    proj[14] = 1e-3;  // cur.inverse with another bottom row
    b.mat(128, proj);
    motion_record(a.b.get(), b.b.get(), m);
    if (m[21] != 2.0) rc |= fail("a projective inverse gives no history");
    place(b, 0.125, NAN, 0, 0);
    motion_record(a.b.get(), b.b.get(), m);
    if (m[21] != 2.0) rc |= fail("a NaN gives no history");

    // identity: spheres compare by type alone; a group by its roots and box, childCount clamped to the record
    Record g0, g1;
    g0.type(4), g1.type(4);
    g0.children(kMaxChildren, 3), g1.children(kMaxChildren, 3);
    g0.box(-1, 1), g1.box(-1, 1);
    if (identity_change(object_identity(g0.b.get()), object_identity(g1.b.get()))) rc |= fail("equal groups");
    place(g1, 0.5, 1, 2, 3);  // a transform is no part of the identity
    if (identity_change(object_identity(g0.b.get()), object_identity(g1.b.get()))) rc |= fail("a moved group");
    g1.children(kMaxChildren, 4);
    if (!identity_change(object_identity(g0.b.get()), object_identity(g1.b.get()))) rc |= fail("changed roots");
    g1.children(kMaxChildren, 3), g1.box(-1, 1.5);
    if (!identity_change(object_identity(g0.b.get()), object_identity(g1.b.get()))) rc |= fail("a changed box");
    g1.box(-1, 1), g1.children(2, 3);
    if (!identity_change(object_identity(g0.b.get()), object_identity(g1.b.get()))) rc |= fail("a changed childCount");
    g1.children(0x7fffffff, 3);  // out of range: clamped, never read past the record
    (void)object_identity(g1.b.get());
    g1.children(-5, 3);
    (void)object_identity(g1.b.get());
    g1.type(1);
    if (!identity_change(object_identity(g0.b.get()), object_identity(g1.b.get()))) rc |= fail("a changed type");
    if (identity_change(object_identity(a.b.get()), object_identity(b.b.get()))) rc |= fail("spheres keep their identity");

    // a table of 16 records into a buffer of exactly 16 x 24 doubles
    std::vector<double> table(16 * kMotionDoubles);
    for (int k = 0; k < 16; k++) motion_record(a.b.get(), a.b.get(), table.data() + kMotionDoubles * k);
    for (int k = 0; k < 16; k++)
        if (table[kMotionDoubles * k + 21] != 0.0) rc |= fail("a static table");
    std::printf(rc ? "FAILED\n" : "ok\n");
    return rc;
}
