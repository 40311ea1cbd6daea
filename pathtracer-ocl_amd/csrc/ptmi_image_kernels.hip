// ptmi_image_kernels.hip -- gfx950 (MI355X / CDNA4) image-space passes: the a-trous denoiser, temporal
// reprojection, history rectification, variance estimation, the error map and its summaries, accumulate,
// finalize, tile selection, the multi-device combine and seed generation, each with its launch wrapper (ptmi_launch.h).
//
// They work on frames, records and tile lists alone: nothing here sees a scene, a camera or a PTMI_*
// build switch, and the only tie to the path tracer (ptmi_kernels.hip) is the tile size kTile.  Compiled
// with the tracer's flags (-ffp-contract=off: every FP64 operation separately rounded, in the order the
// numpy statements in ptmi/denoise.py, ptmi/temporal.py and ptmi/error.py give).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptmi_device.h"
#include "ptmi_launch.h"

namespace ptmi {

// ---- The a-trous denoiser (ptmi_denoise) ------------------------------------------------------
// An edge-avoiding wavelet filter steered by the first-hit records and the pixels' variance.  The
// state is (r, g, b, var) per pixel, ping-ponged between the two halves of the caller's workspace:
// denoise_start forms it, denoise_pass runs once per step 2^i, denoise_end writes the frame.  Every
// FP64 operation is separately rounded and in the order ptmi/denoise.py atrous_reference states;
// exp is the one operation numpy may round differently.
struct DenoiseArgs {
    int W, H, step, npow;
    double sigma_l, sigma_d;
};
// A tap: its state, and of its record the position, the normal and the object id.
struct DnTap {
    double c0, c1, c2, v, x0, x1, x2, n0, n1, n2, id;
};
__device__ __forceinline__ double dn_lum(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }
__device__ __forceinline__ double dn_floor(double a) { return a > 1e-3 ? a : 1e-3; }  // (NaN: the floor)
__device__ __forceinline__ bool dn_finite(double a, double b, double c, double d) {
    return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

__global__ __launch_bounds__(256) void denoise_start(const double* __restrict__ rgba, const double* __restrict__ se,
                                                     const double* __restrict__ feat, double* __restrict__ state,
                                                     uint32_t npix, bool demod) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double2* p = reinterpret_cast<const double2*>(rgba + 4 * (size_t)i);
    const double2* f = reinterpret_cast<const double2*>(feat + 12 * (size_t)i);
    const double2 p0 = p[0], p1 = p[1], a0 = f[4], a1 = f[5];
    const double s = se[i];
    double r = p0.x, g = p0.y, b = p1.x, v = s * s;
    if (demod) {
        const double m = dn_floor(dn_lum(a0.x, a0.y, a1.x));
        r = r / dn_floor(a0.x);
        g = g / dn_floor(a0.y);
        b = b / dn_floor(a1.x);
        v = v / (m * m);
    }
    double2* o = reinterpret_cast<double2*>(state + 4 * (size_t)i);
    o[0] = make_double2(r, g);
    o[1] = make_double2(b, v);
}

__global__ __launch_bounds__(256) void denoise_end(const double* __restrict__ state, const double* __restrict__ rgba,
                                                   const double* __restrict__ se, const double* __restrict__ feat,
                                                   double* __restrict__ out, double* __restrict__ out_se, uint32_t npix,
                                                   bool demod) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double2* p = reinterpret_cast<const double2*>(rgba + 4 * (size_t)i);
    const double2* q = reinterpret_cast<const double2*>(state + 4 * (size_t)i);
    const double2* f = reinterpret_cast<const double2*>(feat + 12 * (size_t)i);
    const double2 p0 = p[0], p1 = p[1], q0 = q[0], q1 = q[1], a0 = f[4], a1 = f[5];
    const double s = se[i];
    double r = q0.x, g = q0.y, b = q1.x, e = sqrt(q1.y);
    if (demod) {
        r = r * dn_floor(a0.x);
        g = g * dn_floor(a0.y);
        b = b * dn_floor(a1.x);
        e = e * dn_floor(dn_lum(a0.x, a0.y, a1.x));
    }
    if (!dn_finite(p0.x, p0.y, p1.x, s)) r = p0.x, g = p0.y, b = p1.x, e = s;  // such a pixel passes through
    double2* o = reinterpret_cast<double2*>(out + 4 * (size_t)i);
    o[0] = make_double2(r, g);
    o[1] = make_double2(b, 1.0);
    if (out_se) out_se[i] = e;
}

// One pass, one thread per pixel on kDnX x kDnY blocks.  kLdsStep == 0: every tap is a global gather
// (two 16-B loads of state, four of the record).  kLdsStep == 1, 2: the pass at that step with the
// block's pixels and their halo of 2 * step staged in LDS first, 11 planes of doubles; the arithmetic
// is the same, so the two forms give the same bits.
static constexpr int kDnX = 16, kDnY = 16;
template <int kLdsStep>
__global__ __launch_bounds__(kDnX * kDnY) void denoise_pass(const double* __restrict__ sin,
                                                            const double* __restrict__ feat,
                                                            double* __restrict__ sout, DenoiseArgs a) {
    constexpr bool kLds = kLdsStep != 0;
    constexpr int kHalo = 2 * kLdsStep, kTW = kDnX + 2 * kHalo, kTH = kDnY + 2 * kHalo;
    __shared__ double lds[kLds ? 11 : 1][kLds ? kTW * kTH : 1];
    const int W = a.W, H = a.H, step = kLds ? kLdsStep : a.step;
    const int bx0 = (int)blockIdx.x * kDnX, by0 = (int)blockIdx.y * kDnY;
    const int x = bx0 + (int)threadIdx.x % kDnX, y = by0 + (int)threadIdx.x / kDnX;
    auto gtap = [&](int qx, int qy) {
        const size_t i = (size_t)qy * W + qx;
        const double2* s = reinterpret_cast<const double2*>(sin + 4 * i);
        const double2* f = reinterpret_cast<const double2*>(feat + 12 * i);
        const double2 s0 = s[0], s1 = s[1], f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
        return DnTap{s0.x, s0.y, s1.x, s1.y, f0.x, f0.y, f1.x, f2.x, f2.y, f3.x, f3.y};
    };
    if constexpr (kLds) {  // in-image pixels of the tile; the others are never read (their taps are skipped)
        for (int k = (int)threadIdx.x; k < kTW * kTH; k += kDnX * kDnY) {
            const int qx = bx0 - kHalo + k % kTW, qy = by0 - kHalo + k / kTW;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const DnTap T = gtap(qx, qy);
            lds[0][k] = T.c0, lds[1][k] = T.c1, lds[2][k] = T.c2, lds[3][k] = T.v;
            lds[4][k] = T.x0, lds[5][k] = T.x1, lds[6][k] = T.x2;
            lds[7][k] = T.n0, lds[8][k] = T.n1, lds[9][k] = T.n2, lds[10][k] = T.id;
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    auto tap = [&](int qx, int qy) {
        if constexpr (kLds) {
            const int k = (qy - by0 + kHalo) * kTW + (qx - bx0 + kHalo);
            return DnTap{lds[0][k], lds[1][k], lds[2][k], lds[3][k], lds[4][k], lds[5][k],
                         lds[6][k], lds[7][k], lds[8][k], lds[9][k], lds[10][k]};
        } else {
            return gtap(qx, qy);
        }
    };
    // the state and the id alone (the variance prefilter's taps)
    auto tap_s = [&](int qx, int qy) {
        if constexpr (kLds) {
            const int k = (qy - by0 + kHalo) * kTW + (qx - bx0 + kHalo);
            return DnTap{lds[0][k], lds[1][k], lds[2][k], lds[3][k], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, lds[10][k]};
        } else {
            const size_t i = (size_t)qy * W + qx;
            const double2* s = reinterpret_cast<const double2*>(sin + 4 * i);
            const double2 s0 = s[0], s1 = s[1];
            return DnTap{s0.x, s0.y, s1.x, s1.y, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, feat[12 * i + 7]};
        }
    };
    const size_t i = (size_t)y * W + x;
    const DnTap P = tap(x, y);
    double2* o = reinterpret_cast<double2*>(sout + 4 * i);
    if (!dn_finite(P.c0, P.c1, P.c2, P.v)) {  // passes through
        o[0] = make_double2(P.c0, P.c1);
        o[1] = make_double2(P.c2, P.v);
        return;
    }
    const bool miss = P.id < 0.0;
    // the variance around p: 3x3 (1/4, 1/8, 1/16) at distance 1 over the taps the filter itself would take
    double sv = 0.0, sk = 0.0;
#pragma unroll
    for (int gy = 0; gy < 3; gy++) {
#pragma unroll
        for (int gx = 0; gx < 3; gx++) {
            const double k = (gx == 1 ? 0.5 : 0.25) * (gy == 1 ? 0.5 : 0.25);
            const int qx = x + gx - 1, qy = y + gy - 1;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const DnTap Q = tap_s(qx, qy);
            if (!dn_finite(Q.c0, Q.c1, Q.c2, Q.v) || (Q.id < 0.0) != miss) continue;
            sv = sv + k * Q.v;
            sk = sk + k;
        }
    }
    const double vbar = sv / sk;
    const double sd = a.sigma_l * sqrt(vbar < 0.0 ? 0.0 : vbar) + 1e-12;
    const double dd_den = a.sigma_d * feat[12 * i + 3] + 1e-12;
    const double lp = dn_lum(P.c0, P.c1, P.c2);
    double sw = 0.0, s2 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
#pragma unroll
    for (int iy = 0; iy < 5; iy++) {
#pragma unroll
        for (int ix = 0; ix < 5; ix++) {
            const double hx = ix == 2 ? 0.375 : (ix == 1 || ix == 3) ? 0.25 : 0.0625;
            const double hy = iy == 2 ? 0.375 : (iy == 1 || iy == 3) ? 0.25 : 0.0625;
            const double hh = hx * hy;
            const int qx = x + (ix - 2) * step, qy = y + (iy - 2) * step;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const DnTap Q = tap(qx, qy);
            if (!dn_finite(Q.c0, Q.c1, Q.c2, Q.v) || (Q.id < 0.0) != miss) continue;
            double w = hh;
            if (!(ix == 2 && iy == 2)) {
                const double wl = exp(-(fabs(lp - dn_lum(Q.c0, Q.c1, Q.c2)) / sd));
                if (miss) {
                    w = hh * wl;
                } else {
                    const double dn = (P.n0 * Q.n0 + P.n1 * Q.n1) + P.n2 * Q.n2;
                    double wn = dn > 0.0 ? dn : 0.0;
                    for (int k = 0; k < a.npow; k++) wn = wn * wn;
                    const double dd = (P.n0 * (Q.x0 - P.x0) + P.n1 * (Q.x1 - P.x1)) + P.n2 * (Q.x2 - P.x2);
                    const double wd = exp(-(fabs(dd) / dd_den));
                    w = ((hh * wn) * wd) * wl;
                }
            }
            sw = sw + w;
            s2 = s2 + (w * w) * Q.v;
            r0 = r0 + w * (Q.c0 - P.c0);
            r1 = r1 + w * (Q.c1 - P.c1);
            r2 = r2 + w * (Q.c2 - P.c2);
        }
    }
    // the weighted mean written around c_p: equal colours stay equal bit for bit
    o[0] = make_double2(P.c0 + r0 / sw, P.c1 + r1 / sw);
    o[1] = make_double2(P.c2 + r2 / sw, s2 / (sw * sw));
}

// work: two states of npix * 4 doubles.  variant (ptmi_diag_denoise_variant): 0 every pass gathers from
// global memory; 1 the passes at steps 1 and 2 stage their tile in LDS.
hipError_t launch_denoise(const double* rgba, const double* se, const double* feat, uint32_t W, uint32_t H,
                          uint32_t iterations, bool demod, double sigma_l, double sigma_d, uint32_t npow, double* out,
                          double* out_se, double* work, int variant, hipStream_t st) {
    const uint32_t npix = W * H;
    double* cur = work;
    double* nxt = work + 4 * (size_t)npix;
    hipLaunchKernelGGL(denoise_start, dim3((npix + 255) / 256), dim3(256), 0, st, rgba, se, feat, cur, npix, demod);
    const dim3 grid((W + kDnX - 1) / kDnX, (H + kDnY - 1) / kDnY), block(kDnX * kDnY);
    for (uint32_t i = 0; i < iterations; i++) {
        const DenoiseArgs a{(int)W, (int)H, 1 << i, (int)npow, sigma_l, sigma_d};
        if (variant == 1 && i == 0)
            hipLaunchKernelGGL(denoise_pass<1>, grid, block, 0, st, cur, feat, nxt, a);
        else if (variant == 1 && i == 1)
            hipLaunchKernelGGL(denoise_pass<2>, grid, block, 0, st, cur, feat, nxt, a);
        else
            hipLaunchKernelGGL(denoise_pass<0>, grid, block, 0, st, cur, feat, nxt, a);
        double* tmp = cur;
        cur = nxt;
        nxt = tmp;
    }
    hipLaunchKernelGGL(denoise_end, dim3((npix + 255) / 256), dim3(256), 0, st, cur, rgba, se, feat, out, out_se, npix,
                       demod);
    return hipGetLastError();
}

// ---- Temporal accumulation (ptmi_reproject) ----------------------------------------------------
// First the lookup reproject_pass and variance_pass share: the pixel's surface point (px, py, pz; t_p = pt) and
// normal carried back to where they were (kMotion), projected with the previous camera, and the four taps
// (0,0), (1,0), (0,1), (1,1) tested against the previous frame's 8-double records `prev` (a history or a
// moment record: [0..3] finite, [4] > 0) and first-hit records.  tap(w, h0, h1, h2) is called per accepted
// tap, in that order, with its bilinear weight and the first three 16-B pairs of its record; a pixel that
// resets (no usable motion, a point behind the camera) gets no call.  Forced inline: each caller's sums
// stay in registers, in the operation order ptmi/temporal.py _history_taps states.
template <bool kMotion, class Tap>
__device__ __forceinline__ void history_taps(const ReprojectArgs& a, const double* __restrict__ prev,
                                             const double* __restrict__ prev_feat, const double* __restrict__ motion,
                                             int n_obj, double px, double py, double pz, double pt, double n0, double n1,
                                             double n2, double id, Tap&& tap) {
    const int W = a.W, H = a.H;
    // the surface point and its normal as the previous frame saw them
    double ux = px, uy = py, uz = pz, m0 = n0, m1 = n1, m2 = n2;
    bool history = true;
    if (kMotion) {
        if (id < (double)n_obj) {  // (id >= 0 here; a NaN id fails and stays static)
            const double2* mr = reinterpret_cast<const double2*>(motion + 24 * (int)id);
            const double state = mr[10].y;
            if (state == 1.0) {
                const double2 b0 = mr[0], b1 = mr[1], b2 = mr[2], b3 = mr[3], b4 = mr[4], b5 = mr[5];
                const double2 g0 = mr[6], g1 = mr[7], g2 = mr[8], g3 = mr[9], g4 = mr[10];
                ux = ((b0.x * px + b0.y * py) + b1.x * pz) + b1.y;
                uy = ((b2.x * px + b2.y * py) + b3.x * pz) + b3.y;
                uz = ((b4.x * px + b4.y * py) + b5.x * pz) + b5.y;
                const double e0 = (g0.x * n0 + g0.y * n1) + g1.x * n2;
                const double e1 = (g1.y * n0 + g2.x * n1) + g2.y * n2;
                const double e2 = (g3.x * n0 + g3.y * n1) + g4.x * n2;
                const double l = (e0 * e0 + e1 * e1) + e2 * e2;
                history = l > 0.0 && isfinite(l);
                const double len = sqrt(l);
                m0 = e0 / len;
                m1 = e1 / len;
                m2 = e2 / len;
            } else if (state != 0.0) {
                history = false;
            }
        }
    }
    const double* T = a.T;
    const double qx = ((T[0] * ux + T[1] * uy) + T[2] * uz) + T[3];
    const double qy = ((T[4] * ux + T[5] * uy) + T[6] * uz) + T[7];
    const double z = -(((T[8] * ux + T[9] * uy) + T[10] * uz) + T[11]);
    if (!(history && z > 0.0)) return;
    const double fu = (a.half_width - qx / z) / a.pixel_size - 0.5;
    const double fv = (a.half_height - qy / z) / a.pixel_size - 0.5;
    const double fx0 = floor(fu), fy0 = floor(fv);
    const double wx = fu - fx0, wy = fv - fy0;
    const double bound = a.plane_dist * pt;
#pragma unroll
    for (int k = 0; k < 4; k++) {  // taps (0,0), (1,0), (0,1), (1,1)
        const int ti = k & 1, tj = k >> 1;
        const double tx = fx0 + (double)ti, ty = fy0 + (double)tj;
        // in double: a NaN or a huge coordinate fails the test before any conversion
        if (!(tx >= 0.0 && tx < (double)W && ty >= 0.0 && ty < (double)H)) continue;
        const size_t q = (size_t)(int)ty * W + (size_t)(int)tx;
        const double2* hq = reinterpret_cast<const double2*>(prev + 8 * q);
        const double2 h0 = hq[0], h1 = hq[1], h2 = hq[2];
        if (!(h2.x > 0.0) || !dn_finite(h0.x, h0.y, h1.x, h1.y)) continue;
        const double2* fq = reinterpret_cast<const double2*>(prev_feat + 12 * q);
        const double2 g0 = fq[0], g1 = fq[1], g2 = fq[2], g3 = fq[3];
        if (g3.y != id) continue;
        const double dn = (m0 * g2.x + m1 * g2.y) + m2 * g3.x;
        if (!(dn >= a.normal_cos)) continue;
        const double dd = (m0 * (g0.x - ux) + m1 * (g0.y - uy)) + m2 * (g1.x - uz);
        if (!(fabs(dd) <= bound)) continue;
        tap((ti ? wx : 1.0 - wx) * (tj ? wy : 1.0 - wy), h0, h1, h2);
    }
}

// reproject_pass.  One thread per pixel on the denoise passes' 16 x 16 blocks: a wave covers 4 rows of 16 pixels, so
// its own loads and stores are 512-B (frame) and 1-KB (history) runs of 16-B accesses, and its taps
// into the previous frame -- neighbouring pixels project to neighbouring places -- stay within a few
// rows.  Per pixel 136 B of its own frame, up to four taps of 48 B history and 64 B of a record, 64 B
// (+ 40 B) out: bandwidth-bound, no LDS.  Every FP64 operation is separately rounded and in the
// order ptmi/temporal.py reproject_reference states; the matrix, the camera scalars and the
// thresholds are by-value arguments (scalar registers).
//
// kMotion (ptmi_reproject_motion): the pixel's object may have moved since the previous frame.  Its
// motion record (include/ptmi.h ptmi_motion_table, 192 B) is read per lane by the pixel's id -- ids are
// not wave-uniform -- as 16-B vector loads; a moved object's point and normal are carried back to where
// they were (x' = B (x_p, 1), n' = G n_p / |G n_p|) before the projection and the tap tests, a static
// one (or an id outside the table) takes the path below with the current point, bit for bit, and an
// object without a usable motion resets (history_taps).  The instantiation without kMotion ignores the two
// trailing arguments, and its outputs are the plain kernel's bit for bit.
//
// kGather (ptmi_history_gather): the same pass up to the blend, which it leaves to ptmi_rectify -- the
// record is the history as found, (h_c, h_var, h_N), and a pixel that resets writes (c_p, se_p^2, 0): N = 0
// says that no history was found.  h_c, h_var and h_N are the values the blend below takes, by the same
// operations in the same order: one kernel text, and what kGather leaves out is left out at compile time.  It
// ignores out_rgba and out_se.
//
// Sharing the lookup with variance_pass rescheduled all four instantiations by a few instructions
// (profiles/variance/SUMMARY.md): they keep their outputs bit for bit, not the instruction stream they had.
template <bool kMotion, bool kGather>
__global__ __launch_bounds__(kDnX * kDnY) void reproject_pass(const double* __restrict__ rgba,
                                                                const double* __restrict__ se,
                                                                const double* __restrict__ feat,
                                                                const double* __restrict__ prev_hist,
                                                                const double* __restrict__ prev_feat,
                                                                ReprojectArgs a, double* __restrict__ out_hist,
                                                                double* __restrict__ out_rgba,
                                                                double* __restrict__ out_se,
                                                                const double* __restrict__ motion, int n_obj) {
    const int W = a.W, H = a.H;
    const int x = (int)blockIdx.x * kDnX + (int)threadIdx.x % kDnX, y = (int)blockIdx.y * kDnY + (int)threadIdx.x / kDnX;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const double2* p = reinterpret_cast<const double2*>(rgba + 4 * i);
    const double2* f = reinterpret_cast<const double2*>(feat + 12 * i);
    const double2 p0 = p[0], p1 = p[1], f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
    const double s = se[i];
    const double c0 = p0.x, c1 = p0.y, c2 = p1.x;
    const double px = f0.x, py = f0.y, pz = f1.x, pt = f1.y, n0 = f2.x, n1 = f2.y, n2 = f3.x, id = f3.y;
    const double v = s * s;
    const bool fin = dn_finite(c0, c1, c2, s);
    // the reset: this frame alone (a pixel that is not finite is no history for the next frame)
    double o0 = c0, o1 = c1, o2 = c2, ov = v, on = kGather ? 0.0 : fin ? 1.0 : 0.0;
    if (prev_hist != nullptr && fin && !(id < 0.0)) {
        double sw = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0, sv = 0.0, sn = 0.0;
        history_taps<kMotion>(a, prev_hist, prev_feat, motion, n_obj, px, py, pz, pt, n0, n1, n2, id,
                              [&](double w, const double2& h0, const double2& h1, const double2& h2) {
                                  sw = sw + w;
                                  r0 = r0 + w * (h0.x - c0);
                                  r1 = r1 + w * (h0.y - c1);
                                  r2 = r2 + w * (h1.x - c2);
                                  sv = sv + (w * w) * h1.y;
                                  sn = sn + w * h2.x;
                              });
        if (sw >= a.min_weight && sw > 0.0) {  // (a pixel history_taps reset: W = 0)
            // the history's weighted mean written around this frame's colour, and the blend around
            // the history: a constant sequence stays constant bit for bit
            const double h0 = c0 + r0 / sw, h1 = c1 + r1 / sw, h2 = c2 + r2 / sw;
            const double hv = sv / (sw * sw), hn = sn / sw;
            if constexpr (kGather) {
                o0 = h0, o1 = h1, o2 = h2, ov = hv, on = hn;
            } else {
                const double np1 = hn + 1.0;
                on = np1 < a.max_history ? np1 : a.max_history;
                const double al = 1.0 / on, be = 1.0 - al;
                o0 = h0 + al * (c0 - h0);
                o1 = h1 + al * (c1 - h1);
                o2 = h2 + al * (c2 - h2);
                ov = (al * al) * v + (be * be) * hv;
            }
        }
    }
    double2* oh = reinterpret_cast<double2*>(out_hist + 8 * i);
    oh[0] = make_double2(o0, o1);
    oh[1] = make_double2(o2, ov);
    oh[2] = make_double2(on, 0.0);
    oh[3] = make_double2(0.0, 0.0);
    if constexpr (!kGather) {
        if (out_rgba) {
            double2* o = reinterpret_cast<double2*>(out_rgba + 4 * i);
            o[0] = make_double2(o0, o1);
            o[1] = make_double2(o2, 1.0);
        }
        if (out_se) out_se[i] = sqrt(ov);
    }
}

hipError_t launch_reproject(const double* rgba, const double* se, const double* feat, const double* prev_hist,
                            const double* prev_feat, const ReprojectArgs& a, double* out_hist, double* out_rgba,
                            double* out_se, const double* motion, int32_t n_obj, hipStream_t st) {
    const dim3 grid(((uint32_t)a.W + kDnX - 1) / kDnX, ((uint32_t)a.H + kDnY - 1) / kDnY), block(kDnX * kDnY);
    if (motion)
        hipLaunchKernelGGL((reproject_pass<true, false>), grid, block, 0, st, rgba, se, feat, prev_hist, prev_feat, a, out_hist,
                           out_rgba, out_se, motion, (int)n_obj);
    else
        hipLaunchKernelGGL((reproject_pass<false, false>), grid, block, 0, st, rgba, se, feat, prev_hist, prev_feat, a, out_hist,
                           out_rgba, out_se, motion, 0);
    return hipGetLastError();
}

hipError_t launch_history_gather(const double* rgba, const double* se, const double* feat, const double* prev_hist,
                                 const double* prev_feat, const ReprojectArgs& a, double* gathered,
                                 const double* motion, int32_t n_obj, hipStream_t st) {
    const dim3 grid(((uint32_t)a.W + kDnX - 1) / kDnX, ((uint32_t)a.H + kDnY - 1) / kDnY), block(kDnX * kDnY);
    if (motion)
        hipLaunchKernelGGL((reproject_pass<true, true>), grid, block, 0, st, rgba, se, feat, prev_hist, prev_feat, a,
                           gathered, nullptr, nullptr, motion, (int)n_obj);
    else
        hipLaunchKernelGGL((reproject_pass<false, true>), grid, block, 0, st, rgba, se, feat, prev_hist, prev_feat, a,
                           gathered, nullptr, nullptr, motion, 0);
    return hipGetLastError();
}

// ---- History rectification (ptmi_rectify) ------------------------------------------------------
// The gathered history (ptmi_history_gather) tested against this frame over a (2 kR + 1)^2 window of
// pixels on the same object, corrected by the offset found, and blended as reproject_pass blends.  Every
// FP64 operation is separately rounded and in the order ptmi/temporal.py rectify_reference states.
//
// One thread per pixel on the 16 x 16 blocks.  The block and its halo of kR are staged in LDS as ten
// planes of doubles -- colour x 3, se^2, h x 3, h_var, N, id -- and each thread walks its taps from there
// (a global gather would read 49 x 80 B per pixel at kR = 3).  N is staged as 0 for an entry outside the
// image or whose colour or se is not finite: a tap is accepted on N > 0 and an equal id alone, and of an
// entry outside the image nothing else is written or used.
//
// Layout: rows of kRcPitch = 24 doubles in every plane, whatever kR (16 + 2 kR <= 24).  ds_read_b64 banks
// by (address / 4) mod 64 -- 32 doubles -- within each 32-lane half of a wave, and a half reads two rows of
// 16 consecutive doubles.  The four rows of a wave go to its 16-lane groups in the order 0, 2, 1, 3, so a
// half's rows are two apart: 48 doubles = 16 mod 32, the two runs of 16 fill the 32 banks once, and no
// tap read conflicts at any kR or tap offset (adjacent rows, 24 apart, would share 8 banks).  At kR = 4
// the planes are 24 x 24 x 10 x 8 B = 46 KB, three blocks per CU; at kR = 1, 34.6 KB.
struct RcPlane {
    enum { c0, c1, c2, v, h0, h1, h2, hv, n, id, count };
};
static constexpr int kRcPitch = 24;
template <int kR>
__global__ __launch_bounds__(kDnX * kDnY) void rectify_pass(const double* __restrict__ rgba,
                                                              const double* __restrict__ se,
                                                              const double* __restrict__ feat,
                                                              const double* __restrict__ gathered, RectifyArgs a,
                                                              double* __restrict__ out_hist,
                                                              double* __restrict__ out_rgba,
                                                              double* __restrict__ out_se) {
    constexpr int kTW = kDnX + 2 * kR, kTH = kDnY + 2 * kR;
    static_assert(kTW <= kRcPitch, "a tile row fits the pitch");
    __shared__ double lds[RcPlane::count][kTH * kRcPitch];
    const int W = a.W, H = a.H;
    const int bx0 = (int)blockIdx.x * kDnX, by0 = (int)blockIdx.y * kDnY;
    for (int k = (int)threadIdx.x; k < kTW * kTH; k += kDnX * kDnY) {
        const int tx = k % kTW, ty = k / kTW, e = ty * kRcPitch + tx;
        const int qx = bx0 - kR + tx, qy = by0 - kR + ty;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) {
            lds[RcPlane::n][e] = 0.0;
            continue;
        }
        const size_t q = (size_t)qy * W + qx;
        const double2* p = reinterpret_cast<const double2*>(rgba + 4 * q);
        const double2* g = reinterpret_cast<const double2*>(gathered + 8 * q);
        const double2 p0 = p[0], p1 = p[1], g0 = g[0], g1 = g[1], g2 = g[2];
        const double s = se[q];
        lds[RcPlane::c0][e] = p0.x, lds[RcPlane::c1][e] = p0.y, lds[RcPlane::c2][e] = p1.x, lds[RcPlane::v][e] = s * s;
        lds[RcPlane::h0][e] = g0.x, lds[RcPlane::h1][e] = g0.y, lds[RcPlane::h2][e] = g1.x, lds[RcPlane::hv][e] = g1.y;
        lds[RcPlane::n][e] = dn_finite(p0.x, p0.y, p1.x, s) ? g2.x : 0.0;
        lds[RcPlane::id][e] = feat[12 * q + 7];
    }
    __syncthreads();
    // rows 0, 2, 1, 3 of the wave's four to its 16-lane groups (the layout note above)
    const int lane = (int)threadIdx.x & 63, grp = lane >> 4;
    const int lx = lane & 15, ly = ((int)threadIdx.x >> 6) * 4 + (((grp & 1) << 1) | (grp >> 1));
    const int x = bx0 + lx, y = by0 + ly;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const int ce = (ly + kR) * kRcPitch + (lx + kR);
    const double c0 = lds[RcPlane::c0][ce], c1 = lds[RcPlane::c1][ce], c2 = lds[RcPlane::c2][ce];
    const double v = lds[RcPlane::v][ce], idp = lds[RcPlane::id][ce];
    const double hv = lds[RcPlane::hv][ce], hn = lds[RcPlane::n][ce];  // (hn: 0 where the pixel is not finite)
    const bool fin = dn_finite(c0, c1, c2, se[i]);
    // the resets: this frame alone
    double o0 = c0, o1 = c1, o2 = c2, ov = v, on = fin ? 1.0 : 0.0, rho = 1.0;
    if (fin && hn != 0.0) {
        uint32_t m = 0;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, sv = 0.0, sh = 0.0;
        for (int dy = -kR; dy <= kR; dy++) {
#pragma unroll
            for (int dx = -kR; dx <= kR; dx++) {
                const int e = ce + dy * kRcPitch + dx;
                if (!(lds[RcPlane::n][e] > 0.0) || lds[RcPlane::id][e] != idp) continue;  // (a NaN id matches nothing)
                m = m + 1;
                a0 = a0 + (lds[RcPlane::c0][e] - c0);
                a1 = a1 + (lds[RcPlane::c1][e] - c1);
                a2 = a2 + (lds[RcPlane::c2][e] - c2);
                b0 = b0 + (lds[RcPlane::h0][e] - c0);
                b1 = b1 + (lds[RcPlane::h1][e] - c1);
                b2 = b2 + (lds[RcPlane::h2][e] - c2);
                sv = sv + lds[RcPlane::v][e];
                sh = sh + lds[RcPlane::hv][e];
            }
        }
        double h0 = lds[RcPlane::h0][ce], h1 = lds[RcPlane::h1][ce], h2 = lds[RcPlane::h2][ce], hr = hn;
        if (m >= a.min_count) {
            const double md = (double)m;
            const double d0 = (b0 - a0) / md, d1 = (b1 - a1) / md, d2 = (b2 - a2) / md;
            const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
            const double t2 = a.gamma2 * ((sv + sh) / (md * md));
            if (dd > t2) {  // (a NaN on either side: not rectified)
                rho = sqrt(t2 / dd);
                const double f = 1.0 - rho;
                h0 = h0 - f * d0;
                h1 = h1 - f * d1;
                h2 = h2 - f * d2;
                hr = rho * hn;
            }
        }
        const double np1 = hr + 1.0;
        on = np1 < a.max_history ? np1 : a.max_history;
        const double al = 1.0 / on, be = 1.0 - al;
        o0 = h0 + al * (c0 - h0);
        o1 = h1 + al * (c1 - h1);
        o2 = h2 + al * (c2 - h2);
        ov = (al * al) * v + (be * be) * hv;
    }
    double2* oh = reinterpret_cast<double2*>(out_hist + 8 * i);
    oh[0] = make_double2(o0, o1);
    oh[1] = make_double2(o2, ov);
    oh[2] = make_double2(on, rho);
    oh[3] = make_double2(0.0, 0.0);
    if (out_rgba) {
        double2* o = reinterpret_cast<double2*>(out_rgba + 4 * i);
        o[0] = make_double2(o0, o1);
        o[1] = make_double2(o2, 1.0);
    }
    if (out_se) out_se[i] = sqrt(ov);
}

hipError_t launch_rectify(const double* rgba, const double* se, const double* feat, const double* gathered,
                          const RectifyArgs& a, uint32_t radius, double* out_hist, double* out_rgba, double* out_se,
                          hipStream_t st) {
    const dim3 grid(((uint32_t)a.W + kDnX - 1) / kDnX, ((uint32_t)a.H + kDnY - 1) / kDnY), block(kDnX * kDnY);
    switch (radius) {
        case 1: hipLaunchKernelGGL(rectify_pass<1>, grid, block, 0, st, rgba, se, feat, gathered, a, out_hist, out_rgba, out_se); break;
        case 2: hipLaunchKernelGGL(rectify_pass<2>, grid, block, 0, st, rgba, se, feat, gathered, a, out_hist, out_rgba, out_se); break;
        case 3: hipLaunchKernelGGL(rectify_pass<3>, grid, block, 0, st, rgba, se, feat, gathered, a, out_hist, out_rgba, out_se); break;
        case 4: hipLaunchKernelGGL(rectify_pass<4>, grid, block, 0, st, rgba, se, feat, gathered, a, out_hist, out_rgba, out_se); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- Variance estimation (ptmi_variance_estimate) ----------------------------------------------
// The standard error of this frame's pixels from the moments of each surface point's frames, accumulated
// through reproject_pass's lookup (history_taps: one text, so the two cannot drift), and where that history is
// shorter than min_temporal from a (2 kR + 1)^2 window of same-surface pixels of this frame.  Every FP64
// operation is separately rounded and in the order ptmi/temporal.py variance_reference states.
//
// One thread per pixel on the 16 x 16 blocks, in three steps.
//   1. Each pixel's own frame and record and its four temporal taps come from global memory, as in
//      reproject_pass (200 B in, 72 B out per pixel), and give mu', mu2', N'.
//   2. Only a pixel with N' < min_temporal needs the window.  The waves' ballots meet in LDS, and a block none
//      of whose pixels needs it stages nothing and is done: from frame min_temporal on that is almost every
//      block, and the pass costs what the gather costs.  Staging decides no value, so skipping it cannot
//      change one.
//   3. Otherwise the block and its halo of kR are staged as seven planes of doubles -- colour x 3, id,
//      normal x 3 -- and the pixels that need it walk their taps from there; a wave none of whose lanes needs
//      the window branches over the loop (the lanes' `need` is its exec mask).  An entry outside the image or
//      whose colour is not finite is staged with id = NaN, which matches no id: of such an entry nothing else
//      is written or used.
// Layout: rectify_pass's -- rows of kRcPitch = 24 doubles in every plane, the wave's four rows to its 16-lane
// groups in the order 0, 2, 1, 3.  Its argument does not depend on the number of planes, since one
// ds_read_b64 reads one plane: within a 32-lane half the two rows are 48 doubles = 16 mod 32 apart, the two
// runs of 16 doubles fill the 32 banks once, and no tap read conflicts at any kR or offset.  Seven planes at
// kR = 4 are 24 x 24 x 7 x 8 B = 31.5 KB, five blocks per CU; at kR = 1, 23.6 KB.
struct VrPlane {
    enum { c0, c1, c2, id, n0, n1, n2, count };
};
template <bool kMotion, int kR>
__global__ __launch_bounds__(kDnX * kDnY) void variance_pass(const double* __restrict__ rgba,
                                                               const double* __restrict__ se,
                                                               const double* __restrict__ feat,
                                                               const double* __restrict__ prev_mom,
                                                               const double* __restrict__ prev_feat, VarianceArgs a,
                                                               double* __restrict__ out_mom,
                                                               double* __restrict__ out_se,
                                                               const double* __restrict__ motion, int n_obj) {
    constexpr int kTW = kDnX + 2 * kR, kTH = kDnY + 2 * kR;
    static_assert(kTW <= kRcPitch, "a tile row fits the pitch");
    __shared__ double lds[VrPlane::count][kTH * kRcPitch];
    __shared__ uint32_t wave_need[kDnX * kDnY / 64];
    const int W = a.r.W, H = a.r.H;
    const int bx0 = (int)blockIdx.x * kDnX, by0 = (int)blockIdx.y * kDnY;
    // rows 0, 2, 1, 3 of the wave's four to its 16-lane groups (the layout note above)
    const int lane = (int)threadIdx.x & 63, grp = lane >> 4;
    const int lx = lane & 15, ly = ((int)threadIdx.x >> 6) * 4 + (((grp & 1) << 1) | (grp >> 1));
    const int x = bx0 + lx, y = by0 + ly;
    const bool inside = x < W && y < H;
    const size_t i = inside ? (size_t)y * W + x : 0;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, s = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0, id = 0.0;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0, on = 0.0, src = 0.0, var = 0.0;
    bool fin = false, need = false;
    if (inside) {
        const double2* p = reinterpret_cast<const double2*>(rgba + 4 * i);
        const double2* f = reinterpret_cast<const double2*>(feat + 12 * i);
        const double2 p0 = p[0], p1 = p[1], f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
        c0 = p0.x, c1 = p0.y, c2 = p1.x;
        n0 = f2.x, n1 = f2.y, n2 = f3.x, id = f3.y;
        s = (c0 * c0 + c1 * c1) + c2 * c2;
        fin = isfinite(c0) && isfinite(c1) && isfinite(c2);
        // the reset: this frame alone (a pixel that is not finite is no history for the next frame)
        o0 = c0, o1 = c1, o2 = c2, o3 = s, on = fin ? 1.0 : 0.0;
        if (prev_mom != nullptr && fin && !(id < 0.0)) {
            double sw = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, sn = 0.0;
            history_taps<kMotion>(a.r, prev_mom, prev_feat, motion, n_obj, f0.x, f0.y, f1.x, f1.y, n0, n1, n2, id,
                                  [&](double w, const double2& h0, const double2& h1, const double2& h2) {
                                      sw = sw + w;
                                      r0 = r0 + w * (h0.x - c0);
                                      r1 = r1 + w * (h0.y - c1);
                                      r2 = r2 + w * (h1.x - c2);
                                      r3 = r3 + w * (h1.y - s);
                                      sn = sn + w * h2.x;
                                  });
            if (sw >= a.r.min_weight && sw > 0.0) {
                // plain weighted means written around c and s, and the blend around them: a constant sequence
                // keeps mu' = c and mu2' = s bit for bit
                const double h0 = c0 + r0 / sw, h1 = c1 + r1 / sw, h2 = c2 + r2 / sw, h3 = s + r3 / sw;
                const double np1 = sn / sw + 1.0;
                on = np1 < a.r.max_history ? np1 : a.r.max_history;
                const double al = 1.0 / on;
                o0 = h0 + al * (c0 - h0);
                o1 = h1 + al * (c1 - h1);
                o2 = h2 + al * (c2 - h2);
                o3 = h3 + al * (s - h3);
            }
        }
        if (fin) {
            if (on >= a.min_temporal) {
                const double d = o3 - ((o0 * o0 + o1 * o1) + o2 * o2);
                var = (d < 0.0 ? 0.0 : d) * (on / (on - 1.0));
                src = 1.0;
            } else {
                need = true;
            }
        }
    }
    // does a pixel of the block need the window?
    const unsigned long long wave_mask = __ballot(need);
    if (lane == 0) wave_need[threadIdx.x >> 6] = wave_mask != 0ull ? 1u : 0u;
    __syncthreads();
    if ((wave_need[0] | wave_need[1]) | (wave_need[2] | wave_need[3])) {  // (block-uniform)
        for (int k = (int)threadIdx.x; k < kTW * kTH; k += kDnX * kDnY) {
            const int tx = k % kTW, ty = k / kTW, e = ty * kRcPitch + tx;
            const int qx = bx0 - kR + tx, qy = by0 - kR + ty;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) {
                lds[VrPlane::id][e] = __builtin_nan("");
                continue;
            }
            const size_t q = (size_t)qy * W + qx;
            const double2* p = reinterpret_cast<const double2*>(rgba + 4 * q);
            const double2* f = reinterpret_cast<const double2*>(feat + 12 * q);
            const double2 p0 = p[0], p1 = p[1], f2 = f[2], f3 = f[3];
            lds[VrPlane::c0][e] = p0.x, lds[VrPlane::c1][e] = p0.y, lds[VrPlane::c2][e] = p1.x;
            lds[VrPlane::n0][e] = f2.x, lds[VrPlane::n1][e] = f2.y, lds[VrPlane::n2][e] = f3.x;
            lds[VrPlane::id][e] = isfinite(p0.x) && isfinite(p0.y) && isfinite(p1.x) ? f3.y : __builtin_nan("");
        }
        __syncthreads();
        if (need) {
            const int ce = (ly + kR) * kRcPitch + (lx + kR);
            const bool hit = !(id < 0.0);
            uint32_t m = 0;
            double e0 = 0.0, e1 = 0.0, e2 = 0.0, b = 0.0;
            for (int dy = -kR; dy <= kR; dy++) {
#pragma unroll
                for (int dx = -kR; dx <= kR; dx++) {
                    const int e = ce + dy * kRcPitch + dx;
                    if (lds[VrPlane::id][e] != id) continue;  // (a NaN id matches nothing; misses match misses)
                    if (hit) {
                        const double dn = (n0 * lds[VrPlane::n0][e] + n1 * lds[VrPlane::n1][e]) + n2 * lds[VrPlane::n2][e];
                        if (!(dn >= a.window_normal_cos)) continue;
                    }
                    const double d0 = lds[VrPlane::c0][e] - c0, d1 = lds[VrPlane::c1][e] - c1, d2 = lds[VrPlane::c2][e] - c2;
                    m = m + 1;
                    e0 = e0 + d0;
                    e1 = e1 + d1;
                    e2 = e2 + d2;
                    b = b + ((d0 * d0 + d1 * d1) + d2 * d2);
                }
            }
            if (m >= a.min_count) {
                const double md = (double)m;
                const double g0 = e0 / md, g1 = e1 / md, g2 = e2 / md;
                const double d = b / md - ((g0 * g0 + g1 * g1) + g2 * g2);
                var = (d < 0.0 ? 0.0 : d) * (md / (md - 1.0));
                src = 2.0;
            } else {  // the pixel's own magnitude, unless the frame's samples gave a standard error
                const double sp = se ? se[i] : __builtin_inf();
                var = isfinite(sp) ? sp * sp : s;
                src = 3.0;
            }
        }
    }
    if (!inside) return;
    double2* om = reinterpret_cast<double2*>(out_mom + 8 * i);
    om[0] = make_double2(o0, o1);
    om[1] = make_double2(o2, o3);
    om[2] = make_double2(on, src);
    om[3] = make_double2(var, 0.0);
    out_se[i] = fin ? sqrt(var) : se ? se[i] : __builtin_inf();
}

template <bool kMotion>
static hipError_t launch_variance_r(const double* rgba, const double* se, const double* feat, const double* prev_mom,
                                    const double* prev_feat, const VarianceArgs& a, uint32_t radius, double* out_mom,
                                    double* out_se, const double* motion, int n_obj, hipStream_t st) {
    const dim3 grid(((uint32_t)a.r.W + kDnX - 1) / kDnX, ((uint32_t)a.r.H + kDnY - 1) / kDnY), block(kDnX * kDnY);
    switch (radius) {
        case 1: hipLaunchKernelGGL((variance_pass<kMotion, 1>), grid, block, 0, st, rgba, se, feat, prev_mom, prev_feat, a, out_mom, out_se, motion, n_obj); break;
        case 2: hipLaunchKernelGGL((variance_pass<kMotion, 2>), grid, block, 0, st, rgba, se, feat, prev_mom, prev_feat, a, out_mom, out_se, motion, n_obj); break;
        case 3: hipLaunchKernelGGL((variance_pass<kMotion, 3>), grid, block, 0, st, rgba, se, feat, prev_mom, prev_feat, a, out_mom, out_se, motion, n_obj); break;
        case 4: hipLaunchKernelGGL((variance_pass<kMotion, 4>), grid, block, 0, st, rgba, se, feat, prev_mom, prev_feat, a, out_mom, out_se, motion, n_obj); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_variance(const double* rgba, const double* se, const double* feat, const double* prev_mom,
                           const double* prev_feat, const VarianceArgs& a, uint32_t radius, double* out_mom,
                           double* out_se, const double* motion, int32_t n_obj, hipStream_t st) {
    if (motion)
        return launch_variance_r<true>(rgba, se, feat, prev_mom, prev_feat, a, radius, out_mom, out_se, motion, (int)n_obj, st);
    return launch_variance_r<false>(rgba, se, feat, prev_mom, prev_feat, a, radius, out_mom, out_se, nullptr, 0, st);
}

// ---- error map and accumulate (ptmi_error_map, ptmi_accumulate) ------------------------------
// A pixel's standard error from its sums record (r, g, b, n) and second moment (ptmi/error.py
// error_map_reference restates this operation for operation):
//   n == 0: se = 0 (not owned);  n == 1: se = +inf;  else
//   d = sq / n - ((mr*mr + mg*mg) + mb*mb),  var = max(d, 0) * (n / (n - 1)),  se2 = var / n,  se = sqrt(se2)
// counted: n >= 2 (the pixels the summaries run over).  A NaN d stays NaN.
struct PixelErr {
    double se, se2, mean;
    bool counted;
};
__device__ __forceinline__ PixelErr pixel_err(const double* __restrict__ sums, const double* __restrict__ sq,
                                              size_t i) {
    PixelErr e{0.0, 0.0, 0.0, false};
    const double n = sums[4 * i + 3];
    if (n == 0.0) return e;
    if (n == 1.0) {
        e.se = __builtin_inf();
        return e;
    }
    const double mr = sums[4 * i + 0] / n, mg = sums[4 * i + 1] / n, mb = sums[4 * i + 2] / n;
    const double d = sq[i] / n - ((mr * mr + mg * mg) + mb * mb);
    const double var = (d < 0.0 ? 0.0 : d) * (n / (n - 1.0));
    e.se2 = var / n;
    e.se = sqrt(e.se2);
    e.mean = ((mr + mg) + mb) / 3.0;
    e.counted = true;
    return e;
}
// A fixed-shape tree over the workgroup's kN slots (kN a power of two): the same inputs give the
// same bits.  v[0] sums, v[1] maxima, v[2] sums, v[3] sums.
template <int kN>
__device__ __forceinline__ void err_tree(double (*v)[kN], int t) {
    for (int s = kN / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
            v[0][t] = v[0][t] + v[0][t + s];
            v[1][t] = v[1][t + s] > v[1][t] ? v[1][t + s] : v[1][t];
            v[2][t] = v[2][t] + v[2][t + s];
            v[3][t] = v[3][t] + v[3][t + s];
        }
    }
    __syncthreads();
}
// One wave per 8x8 tile (kTile; raster order): se per pixel, the tile's rms se, and the tile's
// (sum se2, max finite se, sum mean, count) into tile_part for error_stats.
__global__ __launch_bounds__(64) void error_map(const double* __restrict__ sums, const double* __restrict__ sq, int W,
                                                int H, double* __restrict__ se, double* __restrict__ tile_err,
                                                double* __restrict__ tile_part) {
    __shared__ double v[4][64];
    const int t = threadIdx.x, tiles_x = (W + kTile - 1) / kTile;
    const int px = (int)(blockIdx.x % (uint32_t)tiles_x) * kTile + (t & 7);
    const int py = (int)(blockIdx.x / (uint32_t)tiles_x) * kTile + (t >> 3);
    PixelErr e{0.0, 0.0, 0.0, false};
    if (px < W && py < H) {
        const size_t i = (size_t)py * W + px;
        e = pixel_err(sums, sq, i);
        if (se) se[i] = e.se;
    }
    v[0][t] = e.counted ? e.se2 : 0.0;
    v[1][t] = (e.counted && e.se < __builtin_inf()) ? e.se : 0.0;  // (a NaN se compares false)
    v[2][t] = e.counted ? e.mean : 0.0;
    v[3][t] = e.counted ? 1.0 : 0.0;
    err_tree<64>(v, t);
    if (t == 0) {
        if (tile_err) tile_err[blockIdx.x] = v[3][0] > 0.0 ? sqrt(v[0][0] / v[3][0]) : 0.0;
        for (int k = 0; k < 4; k++) tile_part[4 * (size_t)blockIdx.x + k] = v[k][0];
    }
}
// The frame's summaries from the tiles' (one workgroup): thread t folds tiles t, t + 256, ... in
// that order, then the tree.  stats: rms se, max finite se, mean of the pixel means, pixel count.
__global__ __launch_bounds__(256) void error_stats(const double* __restrict__ tile_part, uint32_t tiles,
                                                   double* __restrict__ stats) {
    __shared__ double v[4][256];
    const int t = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (uint32_t k = (uint32_t)t; k < tiles; k += 256u) {
        const double* p = tile_part + 4 * (size_t)k;
        a0 = a0 + p[0];
        a1 = p[1] > a1 ? p[1] : a1;
        a2 = a2 + p[2];
        a3 = a3 + p[3];
    }
    v[0][t] = a0;
    v[1][t] = a1;
    v[2][t] = a2;
    v[3][t] = a3;
    err_tree<256>(v, t);
    if (t == 0) {
        const double cnt = v[3][0];
        stats[0] = cnt > 0.0 ? sqrt(v[0][0] / cnt) : 0.0;
        stats[1] = v[1][0];
        stats[2] = cnt > 0.0 ? v[2][0] / cnt : 0.0;
        stats[3] = cnt;
    }
}
// dst[k] += src[k] (frame sums, counts included, and second moments of successive batches).
__global__ __launch_bounds__(256) void accumulate_sums(double* __restrict__ dst, const double* __restrict__ src,
                                                       size_t n) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[k] = dst[k] + src[k];
}

// colors * (1.0 / samples), alpha 1 (tracer.cl:837, 1184-1187).
__global__ __launch_bounds__(256) void finalize_kernel(const double* __restrict__ sums, double* __restrict__ out,
                                                       uint32_t npix, uint32_t samples) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double w = 1.0 / samples;
    out[4 * (size_t)i + 0] = sums[4 * (size_t)i + 0] * w;
    out[4 * (size_t)i + 1] = sums[4 * (size_t)i + 1] * w;
    out[4 * (size_t)i + 2] = sums[4 * (size_t)i + 2] * w;
    out[4 * (size_t)i + 3] = 1.0;
}

// finalize_kernel with each pixel's own sample count n = sums[4i + 3] (adaptive renders): the same
// multiply by 1.0 / n, so a uniform count gives finalize_kernel's bits; n == 0 -> RGB 0.  Alpha 1.
__global__ __launch_bounds__(256) void finalize_counts(const double* __restrict__ sums,
                                                              double* __restrict__ out, uint32_t npix) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double n = sums[4 * (size_t)i + 3];
    const double w = 1.0 / n;
    out[4 * (size_t)i + 0] = n == 0.0 ? 0.0 : sums[4 * (size_t)i + 0] * w;
    out[4 * (size_t)i + 1] = n == 0.0 ? 0.0 : sums[4 * (size_t)i + 1] * w;
    out[4 * (size_t)i + 2] = n == 0.0 ? 0.0 : sums[4 * (size_t)i + 2] * w;
    out[4 * (size_t)i + 3] = 1.0;
}

// The tiles that still need samples (ptmi_select_tiles): candidate j is in_tiles[j] (or j itself,
// in_tiles == nullptr), kept iff tile_err[candidate] > threshold -- a NaN error and a tie are
// dropped, +inf is kept -- and the kept ones go to out_tiles in candidate order, their number to
// count[0].  One workgroup walks the candidates in blocks of kSelectBlock, in order: each wave
// ballots its 64 keeps, the waves' counts meet in LDS, and a kept candidate's position is the
// running base plus the earlier waves' counts plus the kept lanes below it.  No atomic decides a
// position: equal inputs give equal lists.
constexpr uint32_t kSelectBlock = 1024;
__global__ __launch_bounds__(kSelectBlock) void select_tiles(const double* __restrict__ tile_err,
                                                                    const uint32_t* __restrict__ in_tiles,
                                                                    uint32_t n_in, double threshold,
                                                                    uint32_t* __restrict__ out_tiles,
                                                                    uint32_t* __restrict__ count) {
    __shared__ uint32_t wave_n[kSelectBlock / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t base = 0;
    for (uint32_t b0 = 0; b0 < n_in; b0 += kSelectBlock) {  // (n_in <= 2^31: b0 + t does not wrap)
        const uint32_t j = b0 + t;
        uint32_t tile = 0;
        bool keep = false;
        if (j < n_in) {
            tile = in_tiles ? in_tiles[j] : j;
            keep = tile_err[tile] > threshold;  // (a NaN compares false)
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_n[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t pos = base, total = 0;
        for (uint32_t w = 0; w < kSelectBlock / 64; w++) {
            const uint32_t n = wave_n[w];
            pos += w < wv ? n : 0u;
            total += n;
        }
        if (keep) out_tiles[pos + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = tile;
        base += total;
        __syncthreads();  // wave_n is rewritten by the next block
    }
    if (t == 0) count[0] = base;
}

// ptmi_trace_multi's device-side combine: out = the partial frames parts[0..nparts)
// (each npix*4 doubles, RGB sums, A = sample count) summed in part order, times 1/S,
// alpha 1 (tracer.cl:1184-1187).  out may alias parts[0].
__global__ __launch_bounds__(256) void combine_kernel(const double* parts, uint32_t nparts, size_t npix,
                                                      double* out, uint32_t samples) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const size_t stride = npix * 4;
    double r = parts[4 * i], g = parts[4 * i + 1], b = parts[4 * i + 2];
    for (uint32_t k = 1; k < nparts; k++) {
        const double* p = parts + k * stride + 4 * i;
        r = r + p[0];
        g = g + p[1];
        b = b + p[2];
    }
    const double w = 1.0 / samples;
    out[4 * i + 0] = r * w;
    out[4 * i + 1] = g * w;
    out[4 * i + 2] = b * w;
    out[4 * i + 3] = 1.0;
}

// Seeds with Go rand.Float64 granularity (k / 2^53) from a SplitMix64 stream.
__global__ __launch_bounds__(256) void seeds_kernel(double* __restrict__ seeds, uint32_t n, uint64_t stream) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t z = stream + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    seeds[i] = (double)(z >> 11) * 0x1p-53;
}

// ---- host-side launch wrappers (called from ptmi_api.cpp) ----------------------
// tile_part: 4 doubles per tile of scratch (ptmi_api.cpp ptmi_error_map).
hipError_t launch_error_map(const double* sums, const double* sq, uint32_t W, uint32_t H, double* se, double* tile_err,
                            double* tile_part, double* stats, hipStream_t st) {
    const uint32_t tiles = ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
    hipLaunchKernelGGL(error_map, dim3(tiles), dim3(64), 0, st, sums, sq, (int)W, (int)H, se, tile_err, tile_part);
    hipLaunchKernelGGL(error_stats, dim3(1), dim3(256), 0, st, tile_part, tiles, stats);
    return hipGetLastError();
}

hipError_t launch_accumulate(double* dst, const double* src, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_sums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}

hipError_t launch_finalize(const double* sums, double* out, uint32_t npix, uint32_t samples, hipStream_t st) {
    hipLaunchKernelGGL(finalize_kernel, dim3((npix + 255) / 256), dim3(256), 0, st, sums, out, npix, samples);
    return hipGetLastError();
}

hipError_t launch_finalize_counts(const double* sums, double* out, uint32_t npix, hipStream_t st) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(finalize_counts, dim3((npix + 255) / 256), dim3(256), 0, st, sums, out, npix);
    return hipGetLastError();
}

hipError_t launch_select_tiles(const double* tile_err, const uint32_t* in_tiles, uint32_t n_in, double threshold,
                               uint32_t* out_tiles, uint32_t* count, hipStream_t st) {
    hipLaunchKernelGGL(select_tiles, dim3(1), dim3(kSelectBlock), 0, st, tile_err, in_tiles, n_in, threshold,
                       out_tiles, count);
    return hipGetLastError();
}

hipError_t launch_combine(const double* parts, uint32_t nparts, size_t npix, double* out, uint32_t samples,
                          hipStream_t st) {
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, parts, nparts, npix, out,
                       samples);
    return hipGetLastError();
}

hipError_t launch_seeds(double* seeds, uint32_t n, uint64_t stream, hipStream_t st) {
    hipLaunchKernelGGL(seeds_kernel, dim3((n + 255) / 256), dim3(256), 0, st, seeds, n, stream);
    return hipGetLastError();
}

}  // namespace ptmi
