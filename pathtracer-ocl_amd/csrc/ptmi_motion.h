// ptmi_motion.h -- the host-only half of object updates on a resident scene (ptmi_scene_set_objects,
// ptmi_motion_table): what of a 1024-byte CLObject record a resident scene's traversal index was built
// from and must therefore keep, and the per-object motion record of ptmi_reproject_motion.  Plain C++,
// no device call: ptmi_api.cpp uses it, and tools/motion_driver.cpp runs it alone under sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace ptmi {

constexpr int kObjectBytes = 1024;   // PTMI_OBJECT_BYTES
constexpr int kMotionDoubles = 24;   // PTMI_MOTION_DOUBLES
constexpr int kMaxChildren = 64;     // CLObject::children (ocltracer.go:42)

// The fields of a record an update may not change: the type (the object's slot in the type runs), and
// for a group object its roots and its box, which the traversal index was built from.
struct ObjectIdentity {
    int64_t type;
    int32_t child_count;
    int32_t children[kMaxChildren];
    unsigned char bb[64];  // bb_min, bb_max as bytes (a NaN bound equals itself)
};

inline ObjectIdentity object_identity(const uint8_t* rec) {
    ObjectIdentity id;
    std::memset(&id, 0, sizeof id);
    std::memcpy(&id.type, rec + 456, 8);
    if (id.type != 4) return id;  // only a group's roots and box reach the index
    std::memcpy(&id.child_count, rec + 584, 4);
    const int32_t n = id.child_count < 0 ? 0 : (id.child_count > kMaxChildren ? kMaxChildren : id.child_count);
    std::memcpy(id.children, rec + 588, 4 * (size_t)n);
    std::memcpy(id.bb, rec + 520, 64);
    return id;
}

// nullptr when `now` may replace `was` on a resident scene, else the name of what changed.
inline const char* identity_change(const ObjectIdentity& was, const ObjectIdentity& now) {
    if (was.type != now.type) return "type";
    if (was.type != 4) return nullptr;
    if (was.child_count != now.child_count) return "childCount";
    if (std::memcmp(was.children, now.children, sizeof was.children) != 0) return "child roots";
    if (std::memcmp(was.bb, now.bb, sizeof was.bb) != 0) return "bb_min / bb_max";
    return nullptr;
}

// Record k of ptmi_motion_table from object k's previous and current records (ptmi/temporal.py
// motion_matrices states the same operations):
//   [0..12)  rows 0-2 of B = prev.transform * cur.inverse, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
//            (geom.multiply's order): a current world point -> where that surface point was
//   [12..21) G = L(prev.inverse_transpose) * L(cur.transform)^T, L the upper-left 3 x 3, each entry
//            (a0 b0 + a1 b1) + a2 b2: the same map for normals
//   [21]     0.0 static (the records' three matrices are byte-equal), 2.0 no history (the bottom row of
//            cur.inverse or of prev.transform is not (0, 0, 0, 1) as values, or B or G is not finite),
//            else 1.0 moved;   [22], [23] 0
// Compile without FP contraction (the products and sums are separately rounded).
inline void motion_record(const uint8_t* prev, const uint8_t* cur, double* out) {
    double pt[16], pit[16], ct[16], ci[16];
    std::memcpy(pt, prev, 128);
    std::memcpy(pit, prev + 256, 128);
    std::memcpy(ct, cur, 128);
    std::memcpy(ci, cur + 128, 128);
    bool finite = true;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            const double a0 = pt[4 * r + 0] * ci[0 + c], a1 = pt[4 * r + 1] * ci[4 + c];
            const double a2 = pt[4 * r + 2] * ci[8 + c], a3 = pt[4 * r + 3] * ci[12 + c];
            const double v = ((a0 + a1) + a2) + a3;
            out[4 * r + c] = v;
            finite = finite && std::isfinite(v);
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double a0 = pit[4 * r + 0] * ct[4 * c + 0], a1 = pit[4 * r + 1] * ct[4 * c + 1];
            const double a2 = pit[4 * r + 2] * ct[4 * c + 2];
            const double v = (a0 + a1) + a2;
            out[12 + 3 * r + c] = v;
            finite = finite && std::isfinite(v);
        }
    auto affine_row = [](const double* m) { return m[12] == 0.0 && m[13] == 0.0 && m[14] == 0.0 && m[15] == 1.0; };
    double state = 1.0;
    if (std::memcmp(prev, cur, 384) == 0)
        state = 0.0;
    else if (!affine_row(ci) || !affine_row(pt) || !finite)
        state = 2.0;
    out[21] = state;
    out[22] = out[23] = 0.0;
}

}  // namespace ptmi
