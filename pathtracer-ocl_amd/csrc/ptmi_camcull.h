// ptmi_camcull.h -- per-tile candidate masks of the camera-ray stage.
// Plain C++, the same text for the device pass (ptmi_kernels.hip tile_cull_pass) and for host code
// (ptmi_api.cpp ptmi_diag_tile_cull_host, tests/camcull): + and * separately rounded, sqrt, comparisons.
//
// Without DoF every camera ray of an 8x8 tile starts at DevCamera::origin and its direction is a
// positive multiple of pixel(a, b) - origin, affine in (a, b) = (half_width - pixel_size (x + rx),
// half_height - pixel_size (y + ry)), rx, ry in [0, 1) in both RNG modes (noise3d ends in fract, xcamera
// in 24 bits x 2^-24).  So the tile's rays are the cone over a planar quadrilateral, for every sample and
// until the camera changes.  Bit i of a tile's mask (i < 16: DevScene::planes[i]; 16 + i:
// DevScene::spheres[i]) is cleared only where no ray of that cone can record the object as a candidate
// (a t > EPSILON); "never the winner" clears nothing.  Every test is written so that a NaN keeps the bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ptmi_device.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTMI_HD __host__ __device__
#else
#define PTMI_HD
#endif

namespace ptmi {

constexpr double kCullEps = 0.0001;           // EPSILON (tracer.cl:4; ptmi_kernels.hip kEps)
constexpr double kCullPixelMargin = 0x1p-10;  // the footprint is enlarged by this many pixels on every side
constexpr double kCullPlaneRel = 1e-9;        // a corner's m . v must exceed this x the magnitude sum N
constexpr double kCullCosMargin = 1e-5;       // spheres: margin on the cosines of the angles to +-o
constexpr double kCullCondMax = 0x1p20;       // spheres: magnitude sum / |w| above this keeps the bit

// The four corners of tile (tx, ty)'s enlarged footprint as pixel - origin (v[c][0..2]), formed as
// ray_for_pixel forms it, and V[r]: the sum of the magnitudes of the terms of component r over the tile.
// Every rounding error of component r, here and in the kernel, is below 2^-50 V[r].
struct CullFootprint {
    double v[4][3];
    double V[3];
};
PTMI_HD inline CullFootprint cull_footprint(const DevCamera& cam, int tx, int ty) {
    CullFootprint F;
    const double x0 = (double)(tx * kTile) - kCullPixelMargin, x1 = (double)(tx * kTile + kTile) + kCullPixelMargin;
    const double y0 = (double)(ty * kTile) - kCullPixelMargin, y1 = (double)(ty * kTile + kTile) + kCullPixelMargin;
    const double a0 = cam.half_width - cam.pixel_size * x0, a1 = cam.half_width - cam.pixel_size * x1;
    const double b0 = cam.half_height - cam.pixel_size * y0, b1 = cam.half_height - cam.pixel_size * y1;
    // corners in order round the quadrilateral
    const double ca[4] = {a0, a1, a1, a0}, cb[4] = {b0, b0, b1, b1};
    const double am = fmax(fabs(a0), fabs(a1)), bm = fmax(fabs(b0), fabs(b1));
    const double* m = cam.inv;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 4; c++)
            F.v[c][r] = (((m[4 * r] * ca[c] + m[4 * r + 1] * cb[c]) + (-m[4 * r + 2])) + m[4 * r + 3]) - cam.origin[r];
        F.V[r] = fabs(m[4 * r]) * am + fabs(m[4 * r + 1]) * bm + fabs(m[4 * r + 2]) + fabs(m[4 * r + 3]) + fabs(cam.origin[r]);
    }
    return F;
}

// Plane: dy = row1 . d has, for every ray of the tile, the sign of the stored origin term oy (nonzero),
// so -oy / dy < 0: no candidate.  m . v is affine over the footprint: decided at the four corners.
PTMI_HD inline bool cull_plane(const CullFootprint& F, const double* row1, double oy) {
    // An origin on the plane, or within EPSILON^2 / 2 of it: a candidate needs |dy| > EPSILON and
    // q = -oy / dy > EPSILON, so |oy| > EPSILON^2 (1 - 2^-50) inside the divide core's range (outside it the
    // plane is no candidate, plane_q); an exact zero gives q = +-0 or, for a non-finite reciprocal, NaN.
    if (fabs(oy) < 0.5 * kCullEps * kCullEps) return true;
    if (!(oy > 0.0) && !(oy < 0.0)) return false;
    const double N = fabs(row1[0]) * F.V[0] + fabs(row1[1]) * F.V[1] + fabs(row1[2]) * F.V[2];
    if (!(N < INFINITY)) return false;
    for (int c = 0; c < 4; c++) {
        const double g = (row1[0] * F.v[c][0] + row1[1] * F.v[c][1]) + row1[2] * F.v[c][2];
        if (!((oy > 0.0 ? g : -g) > kCullPlaneRel * N)) return false;
    }
    return true;
}

PTMI_HD inline double cull_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
PTMI_HD inline void cull_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// The largest cosine between a (length L) and a direction of the convex cone over w[0..3] (in order
// round it; lengths wl): 2 when a lies in the cone or the test cannot tell; else it is attained on the
// boundary -- a corner, or the foot of a on an edge's plane where that foot lies between the edge's corners.
PTMI_HD inline double cull_maxcos(const double* a, double L, const double (*w)[3], const double* wl) {
    int pos = 0, neg = 0;
    double best = -2.0;
    for (int i = 0; i < 4; i++) {
        const int j = (i + 1) & 3;
        double n[3], ap[3], t[3];
        cull_cross(w[i], w[j], n);
        const double nn = cull_dot(n, n), an = cull_dot(a, n);
        if (!(nn > 0.0)) return 2.0;
        if (an >= 0.0) pos++;
        if (an <= 0.0) neg++;
        best = fmax(best, cull_dot(a, w[i]) / (L * wl[i]));
        for (int r = 0; r < 3; r++) ap[r] = nn * a[r] - an * n[r];  // nn x the foot of a on the edge's plane
        cull_cross(w[i], ap, t);
        const double s0 = cull_dot(t, n);
        cull_cross(ap, w[j], t);
        const double s1 = cull_dot(t, n);
        if (!(s0 < 0.0) && !(s1 < 0.0)) best = fmax(best, sqrt(fmax(0.0, 1.0 - (an * an) / ((L * L) * nn))));
    }
    if (pos == 4 || neg == 4) return 2.0;
    return best;
}

// Scale+translate sphere: in its object space the rays start at o = M origin + t (ct[0..2], the camera
// terms; ct[3] = |o|^2 - 1) with directions in the cone over w_c = (m0 v_x, m5 v_y, m10 v_z).  A line from
// o misses the unit sphere -- disc < 0 -- iff its angle to +o and to -o exceeds asin(1 / |o|).
PTMI_HD inline bool cull_sphere(const CullFootprint& F, const SphereRec& Q, const double* ct) {
    const double o[3] = {ct[0], ct[1], ct[2]}, c = ct[3];
    const double L2 = cull_dot(o, o);
    if (!(c > 0.0) || !(L2 > 1.0) || !(L2 < INFINITY)) return false;  // the origin is outside the sphere
    const double D[3] = {Q.m0, Q.m5, Q.m10};
    const double S = fabs(D[0]) * F.V[0] + fabs(D[1]) * F.V[1] + fabs(D[2]) * F.V[2];
    double w[4][3], wl[4], u[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 4; k++) {
        for (int r = 0; r < 3; r++) w[k][r] = D[r] * F.v[k][r];
        wl[k] = sqrt(cull_dot(w[k], w[k]));
        if (!(wl[k] > 0.0)) return false;
        for (int r = 0; r < 3; r++) u[r] += w[k][r] / wl[k];
    }
    // The corners lie in the open half-space round u (the cone is convex and pointed), and every
    // unnormalised direction of the footprint -- a convex combination of the corners -- is at least lo long;
    // its rounding errors (below 2^-49 S) then turn it by less than 2^-28: far inside the cosine margin.
    const double ul = sqrt(cull_dot(u, u));
    double lo = INFINITY;
    for (int k = 0; k < 4; k++) lo = fmin(lo, cull_dot(w[k], u));
    if (!(ul > 0.0) || !(lo > 0.0) || !(S * ul <= kCullCondMax * lo)) return false;
    const double L = sqrt(L2), cosb = sqrt(c / L2);
    const double no[3] = {-o[0], -o[1], -o[2]};
    const double lim = cosb - kCullCosMargin;
    return cull_maxcos(o, L, w, wl) < lim && cull_maxcos(no, L, w, wl) < lim;
}

// The mask of tile (tx, ty).  cam_planes / cam_spheres: the camera terms behind the camera record.
// Scenes with more than 16 planes or more than 16 scale+translate spheres get no culling at all, so a
// mask other than ~0 says that every plane and st sphere of the scene has a bit.
PTMI_HD inline uint32_t cull_tile_mask(const DevCamera& cam, const PlaneRec* planes, int n_planes, const SphereRec* spheres,
                                       int n_spheres_st, const double* cam_planes, const double* cam_spheres, int tx,
                                       int ty) {
    uint32_t mask = ~0u;
    if (n_planes > 16 || n_spheres_st > 16) return mask;
    const CullFootprint F = cull_footprint(cam, tx, ty);
    for (int p = 0; p < n_planes; p++)
        if (cull_plane(F, planes[p].row1, cam_planes[p])) mask &= ~(1u << p);
    for (int q = 0; q < n_spheres_st; q++)
        if (cull_sphere(F, spheres[q], cam_spheres + kCamSphere * q)) mask &= ~(1u << (16 + q));
    return mask;
}

// Where the masks live: behind the camera terms in the camera's allocation (cam_record_bytes).
PTMI_HD inline const uint32_t* cull_masks(const DevCamera* camg, int n_planes, int n_spheres_st) {
    return (const uint32_t*)((const double*)(camg + 1) + n_planes + kCamSphere * n_spheres_st);
}

}  // namespace ptmi
