// ptmi_image_args.h -- what the image-space passes (ptmi_image_api.cpp) accept, as pure functions of the caller's
// arguments: the frame-size rule, the buffer table (no output on another buffer, 16-byte alignment) and one
// checker per call that applies the defaults, validates and fills the kernel's argument record.  Host only, no
// HIP in it, so the CPU suite runs it on fake addresses (tests/host_kat/image_args_kat.cpp, tests/test_image_args.py).
#pragma once
#include <cmath>

#include "ptmi_api_internal.h"

namespace ptmi {

// A frame the image kernels index: both sides 1..65536 and at most 2^31 pixels.
inline bool frame_size_ok(uint32_t width, uint32_t height) {
    return width != 0 && height != 0 && width <= 65536 && height <= 65536 && (uint64_t)width * height <= (1ull << 31);
}

inline bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

// One buffer of a call: where, how many doubles, written or only read, and whether the kernel needs it 16-byte
// aligned (it reads or writes it as double2; the scalar ones, the standard errors, need not be).
struct Range {
    const void* p;
    size_t doubles;
    bool out, aligned;
};

// true: no output overlaps an input or another output (the kernels' pointers are __restrict__), and every pointer
// marked aligned is.  NULL rows, the optional buffers a call leaves out, are skipped.
template <size_t N>
bool buffers_ok(const Range (&t)[N]) {
    auto overlap = [](const Range& a, const Range& b) {
        if (!a.p || !b.p) return false;
        const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
        return a0 < b0 + b.doubles * sizeof(double) && b0 < a0 + a.doubles * sizeof(double);
    };
    uintptr_t low_bits = 0;
    for (size_t i = 0; i < N; i++) {
        if (t[i].aligned) low_bits |= (uintptr_t)t[i].p;
        for (size_t j = 0; t[i].out && j < N; j++)
            if (j != i && overlap(t[i], t[j])) return false;
    }
    return (low_bits & 15u) == 0;
}

// A motion table that a call may leave out: the pointer and the object count go together, 1..PTMI_MAX_OBJECTS.
inline int check_optional_motion(const char* who, const double* motion_dev, uint32_t n_obj, char* err, size_t err_len) {
    if ((motion_dev == nullptr) == (n_obj == 0) && n_obj <= PTMI_MAX_OBJECTS) return PTMI_OK;
    set_err(err, err_len, "bad %s arguments (motion table %s, %u objects)", who, motion_dev ? "given" : "NULL", n_obj);
    return PTMI_ERR_ARG;
}

inline size_t denoise_work_bytes(uint32_t width, uint32_t height) {
    return (size_t)width * (size_t)height * 2 * 4 * sizeof(double);  // two (r, g, b, var) states
}

// ptmi_denoise: `p` gets the parameters with the defaults applied.  Its aliasing rule is the older one: the output
// may not BE the input frame, nothing is said of a partial overlap, and out_se_dev may be anywhere.
inline int check_denoise(const double* rgba_dev, const double* se_dev, const double* feat_dev, uint32_t width,
                         uint32_t height, const ptmi_denoise_params* params, const double* out_rgba_dev,
                         const double* /*out_se_dev*/, const void* work_dev, size_t work_bytes, ptmi_denoise_params& p,
                         char* err, size_t err_len) {
    p = params ? *params : ptmi_denoise_params{5, PTMI_DENOISE_DEMODULATE, 4.0, 0.01, 7, 0};
    if (!rgba_dev || !se_dev || !feat_dev || !out_rgba_dev || !work_dev || !frame_size_ok(width, height)) {
        set_err(err, err_len, "bad denoise arguments (%u x %u)", width, height);
        return PTMI_ERR_ARG;
    }
    if (p.iterations < 1 || p.iterations > 8 || (p.flags & ~PTMI_DENOISE_DEMODULATE) || p.normal_power > 16 ||
        !finite_nonneg(p.sigma_l) || !finite_nonneg(p.sigma_d)) {
        set_err(err, err_len, "bad denoise parameters (iterations %u flags %u sigma_l %g sigma_d %g normal_power %u)",
                p.iterations, p.flags, p.sigma_l, p.sigma_d, p.normal_power);
        return PTMI_ERR_ARG;
    }
    if (work_bytes < denoise_work_bytes(width, height)) {
        set_err(err, err_len, "denoise workspace of %zu bytes, %zu needed", work_bytes,
                denoise_work_bytes(width, height));
        return PTMI_ERR_ARG;
    }
    if (out_rgba_dev == rgba_dev || (((uintptr_t)rgba_dev | (uintptr_t)feat_dev | (uintptr_t)out_rgba_dev |
                                      (uintptr_t)work_dev) & 15u)) {
        set_err(err, err_len, "denoise buffers aliased or not 16-byte aligned");
        return PTMI_ERR_ARG;
    }
    return PTMI_OK;
}

// The world-to-camera matrix of a camera record: the FP64 cofactor inverse of its `inverse`
// (ptmi/temporal.py cofactor_inverse states the same operations).  false: singular or not finite.
inline bool cofactor_inverse(const double* m, double* out) {
    auto det3 = [&](const int* r, const int* c) {
        auto a = [&](int i, int j) { return m[4 * r[i] + c[j]]; };
        return (a(0, 0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0))) +
               a(0, 2) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0));
    };
    double adj[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {  // adj[i][j] = (-1)^(i+j) * minor of m without row j and column i
            int r[3], c[3];
            for (int k = 0, a = 0, b = 0; k < 4; k++) {
                if (k != j) r[a++] = k;
                if (k != i) c[b++] = k;
            }
            const double d = det3(r, c);
            adj[4 * i + j] = ((i + j) & 1) ? -d : d;
        }
    const double det = ((m[0] * adj[0] + m[1] * adj[4]) + m[2] * adj[8]) + m[3] * adj[12];
    if (!std::isfinite(det) || det == 0.0) return false;
    for (int k = 0; k < 16; k++) {
        out[k] = adj[k] / det;
        if (!std::isfinite(out[k])) return false;
    }
    return true;
}

// The previous camera's part of a lookup's arguments (ptmi_reproject and its kin, ptmi_variance_estimate):
// rows 0-2 of its world-to-camera matrix and its pixel mapping.  PTMI_ERR_ARG for a record that is singular,
// not finite or of another size than the frame.
inline int previous_camera_args(const char* who, const void* prev_camera, uint32_t width, uint32_t height,
                                ReprojectArgs& a, char* err, size_t err_len) {
    DevCamera cam{};
    if (const int rc = convert_camera((const uint8_t*)prev_camera, cam, err, err_len)) return rc;
    double T[16];
    if ((uint32_t)cam.width != width || (uint32_t)cam.height != height || !cofactor_inverse(cam.inv, T) ||
        !(std::isfinite(cam.pixel_size) && cam.pixel_size > 0.0) || !std::isfinite(cam.half_width) ||
        !std::isfinite(cam.half_height)) {
        set_err(err, err_len, "%s: bad previous camera (%dx%d for a %ux%u frame, singular or non-finite)", who,
                cam.width, cam.height, width, height);
        return PTMI_ERR_ARG;
    }
    std::memcpy(a.T, T, sizeof(a.T));  // rows 0-2: the point's camera-space x, y, z
    a.half_width = cam.half_width;
    a.half_height = cam.half_height;
    a.pixel_size = cam.pixel_size;
    return PTMI_OK;
}

// A lookup's arguments from the frame and the four parameters that ptmi_reproject_params and
// ptmi_variance_params share; then, where there is one, the previous camera's.
inline int lookup_args(const char* who, uint32_t width, uint32_t height, uint32_t max_history, double normal_cos,
                       double plane_dist, double min_weight, const void* prev_camera, ReprojectArgs& a, char* err,
                       size_t err_len) {
    a = ReprojectArgs{};
    a.W = (int32_t)width;
    a.H = (int32_t)height;
    a.max_history = (double)max_history;
    a.normal_cos = normal_cos;
    a.plane_dist = plane_dist;
    a.min_weight = min_weight;
    return prev_camera ? previous_camera_args(who, prev_camera, width, height, a, err, err_len) : PTMI_OK;
}

// ptmi_reproject (motion_dev == NULL, n_obj == 0), ptmi_reproject_motion and ptmi_history_gather (out_hist_dev is
// the gathered record, and there are no other outputs): one set of checks.
inline int check_reproject(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                           const double* prev_hist_dev, const double* prev_feat_dev, const void* prev_camera,
                           uint32_t width, uint32_t height, const ptmi_reproject_params* params,
                           const double* out_hist_dev, const double* out_rgba_dev, const double* out_se_dev,
                           const double* motion_dev, uint32_t n_obj, ReprojectArgs& a, char* err, size_t err_len) {
    const ptmi_reproject_params p = params ? *params : ptmi_reproject_params{32, 0, 0.9, 0.02, 0.05};
    if (!rgba_dev || !se_dev || !feat_dev || !out_hist_dev || (prev_hist_dev && (!prev_feat_dev || !prev_camera)) ||
        !frame_size_ok(width, height)) {
        set_err(err, err_len, "bad reproject arguments (%u x %u)", width, height);
        return PTMI_ERR_ARG;
    }
    if (p.max_history < 1 || p.max_history > 65536 || p.flags != 0 || !finite_nonneg(p.normal_cos) ||
        !finite_nonneg(p.plane_dist) || !finite_nonneg(p.min_weight)) {
        set_err(err, err_len, "bad reproject parameters (max_history %u flags %u normal_cos %g plane_dist %g min_weight %g)",
                p.max_history, p.flags, p.normal_cos, p.plane_dist, p.min_weight);
        return PTMI_ERR_ARG;
    }
    const size_t npix = (size_t)width * height;
    const Range buffers[] = {{rgba_dev, npix * 4, false, true}, {se_dev, npix, false, false},
                             {feat_dev, npix * PTMI_FEATURE_DOUBLES, false, true},
                             {prev_hist_dev, npix * PTMI_HISTORY_DOUBLES, false, true},
                             {prev_feat_dev, npix * PTMI_FEATURE_DOUBLES, false, true},
                             {motion_dev, (size_t)n_obj * PTMI_MOTION_DOUBLES, false, true},
                             {out_hist_dev, npix * PTMI_HISTORY_DOUBLES, true, true},
                             {out_rgba_dev, npix * 4, true, true}, {out_se_dev, npix, true, false}};
    if (!buffers_ok(buffers)) {
        set_err(err, err_len, "reproject buffers overlap or are not 16-byte aligned");
        return PTMI_ERR_ARG;
    }
    return lookup_args("reproject", width, height, p.max_history, p.normal_cos, p.plane_dist, p.min_weight, prev_camera,
                       a, err, err_len);
}

// ptmi_rectify: also gives the window radius, which is a launch argument and not part of RectifyArgs.
inline int check_rectify(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                         const double* gathered_dev, uint32_t width, uint32_t height, const ptmi_rectify_params* params,
                         const double* out_hist_dev, const double* out_rgba_dev, const double* out_se_dev,
                         RectifyArgs& a, uint32_t& radius, char* err, size_t err_len) {
    const ptmi_rectify_params p = params ? *params : ptmi_rectify_params{3, 9, 3.0, 32, 0};
    if (!rgba_dev || !se_dev || !feat_dev || !gathered_dev || !out_hist_dev || !frame_size_ok(width, height)) {
        set_err(err, err_len, "bad rectify arguments (%u x %u)", width, height);
        return PTMI_ERR_ARG;
    }
    if (p.radius < 1 || p.radius > 4 || !finite_nonneg(p.gamma) || p.max_history < 1 || p.max_history > 65536 ||
        p.flags != 0) {
        set_err(err, err_len, "bad rectify parameters (radius %u min_count %u gamma %g max_history %u flags %u)", p.radius,
                p.min_count, p.gamma, p.max_history, p.flags);
        return PTMI_ERR_ARG;
    }
    const size_t npix = (size_t)width * height;
    const Range buffers[] = {{rgba_dev, npix * 4, false, true}, {se_dev, npix, false, false},
                             {feat_dev, npix * PTMI_FEATURE_DOUBLES, false, true},
                             {gathered_dev, npix * PTMI_HISTORY_DOUBLES, false, true},
                             {out_hist_dev, npix * PTMI_HISTORY_DOUBLES, true, true},
                             {out_rgba_dev, npix * 4, true, true}, {out_se_dev, npix, true, false}};
    if (!buffers_ok(buffers)) {
        set_err(err, err_len, "rectify buffers overlap or are not 16-byte aligned");
        return PTMI_ERR_ARG;
    }
    a = RectifyArgs{};
    a.W = (int32_t)width;
    a.H = (int32_t)height;
    a.min_count = p.min_count;
    a.gamma2 = p.gamma * p.gamma;
    a.max_history = (double)p.max_history;
    radius = p.radius;
    return PTMI_OK;
}

// ptmi_variance_estimate: also gives the window radius (a launch argument).
inline int check_variance(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                          const double* prev_mom_dev, const double* prev_feat_dev, const void* prev_camera,
                          uint32_t width, uint32_t height, const ptmi_variance_params* params,
                          const double* out_mom_dev, const double* out_se_dev, const double* motion_dev, uint32_t n_obj,
                          VarianceArgs& a, uint32_t& radius, char* err, size_t err_len) {
    const ptmi_variance_params p = params ? *params : ptmi_variance_params{32, 4, 3, 9, 0, 0.9, 0.02, 0.05, 0.9};
    if (!rgba_dev || !feat_dev || !out_mom_dev || !out_se_dev || (prev_mom_dev && (!prev_feat_dev || !prev_camera)) ||
        !frame_size_ok(width, height)) {
        set_err(err, err_len, "bad variance_estimate arguments (%u x %u)", width, height);
        return PTMI_ERR_ARG;
    }
    if (const int rc = check_optional_motion("variance_estimate", motion_dev, n_obj, err, err_len)) return rc;
    if (p.max_history < 1 || p.max_history > 65536 || p.min_temporal < 2 || p.min_temporal > 65536 || p.radius < 1 ||
        p.radius > 4 || p.min_count < 2 || p.flags != 0 || !finite_nonneg(p.normal_cos) ||
        !finite_nonneg(p.plane_dist) || !finite_nonneg(p.min_weight) || !finite_nonneg(p.window_normal_cos)) {
        set_err(err, err_len,
                "bad variance parameters (max_history %u min_temporal %u radius %u min_count %u flags %u normal_cos %g "
                "plane_dist %g min_weight %g window_normal_cos %g)",
                p.max_history, p.min_temporal, p.radius, p.min_count, p.flags, p.normal_cos, p.plane_dist, p.min_weight,
                p.window_normal_cos);
        return PTMI_ERR_ARG;
    }
    const size_t npix = (size_t)width * height;
    const Range buffers[] = {{rgba_dev, npix * 4, false, true}, {se_dev, npix, false, false},
                             {feat_dev, npix * PTMI_FEATURE_DOUBLES, false, true},
                             {prev_mom_dev, npix * PTMI_MOMENT_DOUBLES, false, true},
                             {prev_feat_dev, npix * PTMI_FEATURE_DOUBLES, false, true},
                             {motion_dev, (size_t)n_obj * PTMI_MOTION_DOUBLES, false, true},
                             {out_mom_dev, npix * PTMI_MOMENT_DOUBLES, true, true}, {out_se_dev, npix, true, false}};
    if (!buffers_ok(buffers)) {
        set_err(err, err_len, "variance_estimate buffers overlap or are not 16-byte aligned");
        return PTMI_ERR_ARG;
    }
    a = VarianceArgs{};
    a.min_temporal = (double)p.min_temporal;
    a.window_normal_cos = p.window_normal_cos;
    a.min_count = p.min_count;
    radius = p.radius;
    return lookup_args("variance_estimate", width, height, p.max_history, p.normal_cos, p.plane_dist, p.min_weight,
                       prev_camera, a.r, err, err_len);
}

}  // namespace ptmi
