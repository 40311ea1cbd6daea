// Test-only: what the image passes' argument checks (csrc/ptmi_image_args.h) ACCEPT, asked of the checkers
// directly on fake addresses -- the library itself can only be asked on a CPU what it refuses
// (tests/golden/image_arg_errors.json).  Every expectation is read off the conditions the entry points had while
// the checks were written out in ptmi_api.cpp (commit 8b4c6bf), not off the header.  One PASS / FAIL line per case.
#include <cfloat>
#include <cstdio>
#include <string>
#include <vector>

#include "../../pathtracer-ocl_amd/csrc/ptmi_image_args.h"

using namespace ptmi;

static int failures = 0;
static void expect(const std::string& name, bool ok) {
    std::printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
    failures += !ok;
}

constexpr uintptr_t A = 0x100000;  // further apart than the largest W x H buffer, 36 x 20 x 96 bytes
constexpr uintptr_t B = (uintptr_t)1 << 40;  // ... than the largest of a 2^31-pixel frame, 2^31 x 96 bytes
constexpr uint32_t W = 36, H = 20;
constexpr size_t NPIX = (size_t)W * H;
static const double* D(uintptr_t v) { return (const double*)v; }

// A camera record whose `inverse` [2 0 0 1; 0 4 0 2; 0 0 .5 3; 0 0 0 1] has the inverse
// [.5 0 0 -.5; 0 .25 0 -.5; 0 0 2 -6; 0 0 0 1], every cofactor and quotient exact.
static const double kT[12] = {0.5, 0, 0, -0.5, 0, 0.25, 0, -0.5, 0, 0, 2, -6};
struct Camera {
    alignas(8) uint8_t b[PTMI_CAMERA_BYTES] = {};
    Camera(int32_t w = W, int32_t h = H) {
        const double f[5] = {0.125, 2.25, 1.25, 0.0, 1.0};  // pixel_size, half_width, half_height, aperture, focal_length
        const double inv[16] = {2, 0, 0, 1, 0, 4, 0, 2, 0, 0, 0.5, 3, 0, 0, 0, 1};
        std::memcpy(b, &w, 4), std::memcpy(b + 4, &h, 4), std::memcpy(b + 16, f, sizeof f), std::memcpy(b + 56, inv, sizeof inv);
    }
};
static const Camera kCamera;
static bool lookup_filled(const ReprojectArgs& a, bool camera) {
    for (int k = 0; k < 12; k++)
        if (a.T[k] != (camera ? kT[k] : 0.0)) return false;
    return a.W == (int32_t)W && a.H == (int32_t)H && a.half_width == (camera ? 2.25 : 0.0) &&
           a.half_height == (camera ? 1.25 : 0.0) && a.pixel_size == (camera ? 0.125 : 0.0);
}

static char g_err[256];

struct Denoise {
    uintptr_t rgba = A, se = 2 * A, feat = 3 * A, out_rgba = 6 * A, out_se = 7 * A, work = 8 * A;
    uint32_t w = W, h = H;
    ptmi_denoise_params q{5, PTMI_DENOISE_DEMODULATE, 4.0, 0.01, 7, 0}, p{};
    bool defaults = true;
    size_t work_bytes = NPIX * 64;
    int run() {
        return check_denoise(D(rgba), D(se), D(feat), w, h, defaults ? nullptr : &q, D(out_rgba), D(out_se), (void*)work,
                             work_bytes, p, g_err, sizeof g_err);
    }
};
struct Reproject {
    uintptr_t rgba = A, se = 2 * A, feat = 3 * A, prev_hist = 4 * A, prev_feat = 5 * A, out_hist = 6 * A, out_rgba = 7 * A,
              out_se = 8 * A, motion = 0;
    const void* camera = kCamera.b;
    uint32_t w = W, h = H, n_obj = 0;
    ptmi_reproject_params q{32, 0, 0.9, 0.02, 0.05};
    bool defaults = true;
    ReprojectArgs a{};
    int run() {
        return check_reproject(D(rgba), D(se), D(feat), D(prev_hist), D(prev_feat), camera, w, h, defaults ? nullptr : &q,
                               D(out_hist), D(out_rgba), D(out_se), D(motion), n_obj, a, g_err, sizeof g_err);
    }
};
struct Rectify {
    uintptr_t rgba = A, se = 2 * A, feat = 3 * A, gathered = 4 * A, out_hist = 6 * A, out_rgba = 7 * A, out_se = 8 * A;
    uint32_t w = W, h = H, radius = 0;
    ptmi_rectify_params q{3, 9, 3.0, 32, 0};
    bool defaults = true;
    RectifyArgs a{};
    int run() {
        return check_rectify(D(rgba), D(se), D(feat), D(gathered), w, h, defaults ? nullptr : &q, D(out_hist), D(out_rgba),
                             D(out_se), a, radius, g_err, sizeof g_err);
    }
};
struct Variance {
    uintptr_t rgba = A, se = 2 * A, feat = 3 * A, prev_mom = 4 * A, prev_feat = 5 * A, out_mom = 6 * A, out_se = 7 * A,
              motion = 8 * A;
    const void* camera = kCamera.b;
    uint32_t w = W, h = H, n_obj = 3, radius = 0;
    ptmi_variance_params q{32, 4, 3, 9, 0, 0.9, 0.02, 0.05, 0.9};
    bool defaults = true;
    VarianceArgs a{};
    int run() {
        return check_variance(D(rgba), D(se), D(feat), D(prev_mom), D(prev_feat), camera, w, h, defaults ? nullptr : &q,
                              D(out_mom), D(out_se), D(motion), n_obj, a, radius, g_err, sizeof g_err);
    }
};

// The call `Call` with `edit` applied is accepted / refused with PTMI_ERR_ARG.
#define ACCEPTED(Call, name, edit)                                   \
    do {                                                             \
        Call c;                                                      \
        edit;                                                        \
        expect(#Call ": accepts " name, c.run() == PTMI_OK);         \
    } while (0)
#define REFUSED(Call, name, edit)                                    \
    do {                                                             \
        Call c;                                                      \
        edit;                                                        \
        expect(#Call ": refuses " name, c.run() == PTMI_ERR_ARG);    \
    } while (0)
// ... a parameter at both ends of its range
#define ENDS(Call, field, lo, hi)                                                  \
    do {                                                                           \
        ACCEPTED(Call, #field " = " #lo, (c.defaults = false, c.q.field = lo));    \
        ACCEPTED(Call, #field " = " #hi, (c.defaults = false, c.q.field = hi));    \
    } while (0)

// What the four calls share: 8-mod-16 standard errors, the largest frame, buffers that touch.  `out` is the
// call's history-like output of 8 doubles per pixel and `in` the input of that size.
#define COMMON(Call, out, in)                                                                                       \
    do {                                                                                                            \
        ACCEPTED(Call, "the baseline", (void)0);                                                                    \
        ACCEPTED(Call, "se_dev and out_se_dev at 8 mod 16", (c.se += 8, c.out_se += 8));                            \
        ACCEPTED(Call, #out " ending on the byte where " #in " begins", c.out = c.in - NPIX * 64);                  \
        ACCEPTED(Call, #out " beginning on the byte where " #in " ends", c.out = c.in + NPIX * 64);                 \
        REFUSED(Call, #out " ending 16 bytes into " #in, c.out = c.in - NPIX * 64 + 16);                            \
        REFUSED(Call, #out " beginning 16 bytes before the end of " #in, c.out = c.in + NPIX * 64 - 16);            \
        ACCEPTED(Call, "out_se_dev ending where rgba_dev begins", c.out_se = c.rgba - NPIX * 8);                    \
        ACCEPTED(Call, "out_se_dev beginning where se_dev ends", c.out_se = c.se + NPIX * 8);                       \
        ACCEPTED(Call, "65536 x 32768 pixels", (big(c), c.w = 65536, c.h = 32768));                                 \
        REFUSED(Call, "65536 x 32769 pixels", (big(c), c.w = 65536, c.h = 32769));                                  \
        REFUSED(Call, "65537 x 1 pixels", (c.w = 65537, c.h = 1));                                                  \
        REFUSED(Call, "1 x 65537 pixels", (c.w = 1, c.h = 65537));                                                  \
        ACCEPTED(Call, "65536 x 1 pixels", (spread(c), c.camera_size(65536, 1), c.w = 65536, c.h = 1));             \
        ACCEPTED(Call, "1 x 65536 pixels", (spread(c), c.camera_size(1, 65536), c.w = 1, c.h = 65536));             \
    } while (0)

// The same call with its buffers 2^40 apart; big: also without a previous camera (whose size would not match).
template <typename C>
static void spread(C& c) {
    for (uintptr_t* p : c.pointers())
        if (*p) *p = *p / A * B;
}
template <typename C>
static void big(C& c) {
    spread(c);
    c.no_history();
}

struct DenoiseC : Denoise {
    std::vector<uintptr_t*> pointers() { return {&rgba, &se, &feat, &out_rgba, &out_se, &work}; }
    void no_history() { work_bytes = denoise_work_bytes(65536, 32769); }  // (enough for every size asked below)
};
struct ReprojectC : Reproject {
    Camera other;
    std::vector<uintptr_t*> pointers() {
        return {&rgba, &se, &feat, &prev_hist, &prev_feat, &out_hist, &out_rgba, &out_se, &motion};
    }
    void no_history() { prev_hist = prev_feat = 0, camera = nullptr; }
    void camera_size(int32_t cw, int32_t ch) { other = Camera(cw, ch), camera = other.b; }
};
struct RectifyC : Rectify {
    std::vector<uintptr_t*> pointers() { return {&rgba, &se, &feat, &gathered, &out_hist, &out_rgba, &out_se}; }
    void no_history() {}
    void camera_size(int32_t, int32_t) {}
};
struct VarianceC : Variance {
    Camera other;
    std::vector<uintptr_t*> pointers() {
        return {&rgba, &se, &feat, &prev_mom, &prev_feat, &out_mom, &out_se, &motion};
    }
    void no_history() { prev_mom = prev_feat = 0, camera = nullptr; }
    void camera_size(int32_t cw, int32_t ch) { other = Camera(cw, ch), camera = other.b; }
};

int main() {
    expect("frame_size_ok: 1 x 1, 65536 x 32768, 32768 x 65536",
           frame_size_ok(1, 1) && frame_size_ok(65536, 32768) && frame_size_ok(32768, 65536));
    expect("frame_size_ok: not 0 x 1, 1 x 0, 65537 x 1, 65536 x 32769, 65536 x 65536",
           !frame_size_ok(0, 1) && !frame_size_ok(1, 0) && !frame_size_ok(65537, 1) && !frame_size_ok(65536, 32769) &&
               !frame_size_ok(65536, 65536));

    // ---- the optional motion table of ptmi_history_gather and ptmi_variance_estimate
    expect("motion: accepts none, 1 and 16 objects",
           check_optional_motion("x", nullptr, 0, g_err, sizeof g_err) == PTMI_OK &&
               check_optional_motion("x", D(A), 1, g_err, sizeof g_err) == PTMI_OK &&
               check_optional_motion("x", D(A), PTMI_MAX_OBJECTS, g_err, sizeof g_err) == PTMI_OK);
    expect("motion: refuses a table of 0 or 17 objects and objects without a table",
           check_optional_motion("x", D(A), 0, g_err, sizeof g_err) == PTMI_ERR_ARG &&
               check_optional_motion("x", D(A), 17, g_err, sizeof g_err) == PTMI_ERR_ARG &&
               check_optional_motion("history_gather", nullptr, 3, g_err, sizeof g_err) == PTMI_ERR_ARG &&
               std::string(g_err) == "bad history_gather arguments (motion table NULL, 3 objects)");

    // ---- ptmi_denoise: the equality rule, four aligned pointers, no range test
    ACCEPTED(DenoiseC, "the baseline", (void)0);
    ACCEPTED(DenoiseC, "out_se_dev NULL", c.out_se = 0);
    ACCEPTED(DenoiseC, "se_dev and out_se_dev at 8 mod 16", (c.se += 8, c.out_se += 8));
    ACCEPTED(DenoiseC, "out_se_dev inside rgba_dev, feat_dev, out_rgba_dev or the workspace",
             c.out_se = c.rgba + 64; expect("... (rgba_dev)", c.run() == PTMI_OK); c.out_se = c.feat + 8;
             expect("... (feat_dev)", c.run() == PTMI_OK); c.out_se = c.out_rgba; expect("... (out_rgba_dev)", c.run() == PTMI_OK);
             c.out_se = c.work + 16);
    ACCEPTED(DenoiseC, "out_rgba_dev 16 bytes into rgba_dev (only equality is refused)", c.out_rgba = c.rgba + 16);
    REFUSED(DenoiseC, "out_rgba_dev == rgba_dev", c.out_rgba = c.rgba);
    ACCEPTED(DenoiseC, "out_rgba_dev on feat_dev or the workspace (not tested)", c.out_rgba = c.feat; expect("... (feat_dev)", c.run() == PTMI_OK);
             c.out_rgba = c.work);
    ACCEPTED(DenoiseC, "a workspace of exactly ptmi_denoise_work_bytes", c.work_bytes = denoise_work_bytes(W, H));
    REFUSED(DenoiseC, "a workspace one byte short", c.work_bytes = denoise_work_bytes(W, H) - 1);
    ACCEPTED(DenoiseC, "65536 x 32768 pixels", (big(c), c.w = 65536, c.h = 32768));
    REFUSED(DenoiseC, "65536 x 32769 pixels", (big(c), c.w = 65536, c.h = 32769));
    REFUSED(DenoiseC, "65537 x 1 pixels", (c.w = 65537, c.h = 1));
    ENDS(DenoiseC, iterations, 1, 8);
    ENDS(DenoiseC, flags, 0, PTMI_DENOISE_DEMODULATE);
    ENDS(DenoiseC, normal_power, 0, 16);
    ENDS(DenoiseC, sigma_l, 0.0, DBL_MAX);
    ENDS(DenoiseC, sigma_d, 0.0, DBL_MAX);
    ACCEPTED(DenoiseC, "any `reserved`", (c.defaults = false, c.q.reserved = 0xffffffffu));
    REFUSED(DenoiseC, "iterations 0 and 9", (c.defaults = false, c.q.iterations = 0); expect("... (0)", c.run() == PTMI_ERR_ARG);
            c.q.iterations = 9);
    REFUSED(DenoiseC, "normal_power 17", (c.defaults = false, c.q.normal_power = 17));
    {
        DenoiseC c;
        const bool ok = c.run() == PTMI_OK;
        expect("DenoiseC: NULL params give the defaults",
               ok && c.p.iterations == 5 && c.p.flags == PTMI_DENOISE_DEMODULATE && c.p.sigma_l == 4.0 && c.p.sigma_d == 0.01 &&
                   c.p.normal_power == 7);
        c.defaults = false, c.q.iterations = 3, c.q.flags = 0;
        expect("DenoiseC: given params are passed on", c.run() == PTMI_OK && c.p.iterations == 3 && c.p.flags == 0);
    }

    // ---- ptmi_reproject, ptmi_reproject_motion, ptmi_history_gather
    COMMON(ReprojectC, out_hist, prev_hist);
    ACCEPTED(ReprojectC, "out_rgba_dev NULL", c.out_rgba = 0);
    ACCEPTED(ReprojectC, "out_se_dev NULL", c.out_se = 0);
    ACCEPTED(ReprojectC, "only out_hist_dev (ptmi_history_gather)", c.out_rgba = c.out_se = 0);
    ACCEPTED(ReprojectC, "the first frame: no history, no records, no camera", c.no_history();
             expect("... with T = 0", c.run() == PTMI_OK && lookup_filled(c.a, false)));
    ACCEPTED(ReprojectC, "no history but its records and camera", c.prev_hist = 0);
    REFUSED(ReprojectC, "a history without its records", c.prev_feat = 0);
    REFUSED(ReprojectC, "a history without its camera", c.camera = nullptr);
    ACCEPTED(ReprojectC, "a motion table of 8 and of 16 objects", (c.motion = 9 * A, c.n_obj = 8); expect("... (8)", c.run() == PTMI_OK);
             c.n_obj = 16);
    ACCEPTED(ReprojectC, "out_se_dev ending where the motion table begins", (c.motion = 9 * A, c.n_obj = 8, c.out_se = 9 * A - NPIX * 8));
    ACCEPTED(ReprojectC, "out_rgba_dev beginning where the motion table ends",
             (c.motion = 9 * A, c.n_obj = 8, c.out_rgba = 9 * A + 8 * PTMI_MOTION_DOUBLES * 8));
    REFUSED(ReprojectC, "out_se_dev on the motion table's last 8 bytes",
            (c.motion = 9 * A, c.n_obj = 8, c.out_se = 9 * A + 8 * PTMI_MOTION_DOUBLES * 8 - 8));
    REFUSED(ReprojectC, "a motion table at 8 mod 16", (c.motion = 9 * A + 8, c.n_obj = 8));
    ENDS(ReprojectC, max_history, 1, 65536);
    ENDS(ReprojectC, normal_cos, 0.0, DBL_MAX);
    ENDS(ReprojectC, plane_dist, 0.0, DBL_MAX);
    ENDS(ReprojectC, min_weight, 0.0, DBL_MAX);
    REFUSED(ReprojectC, "max_history 0 and 65537", (c.defaults = false, c.q.max_history = 0); expect("... (0)", c.run() == PTMI_ERR_ARG);
            c.q.max_history = 65537);
    REFUSED(ReprojectC, "a camera of another size", c.camera_size(W + 1, H);
            expect("... and says `reproject`", c.run() == PTMI_ERR_ARG &&
                   std::string(g_err) == "reproject: bad previous camera (37x20 for a 36x20 frame, singular or non-finite)"));
    {
        ReprojectC c;
        expect("ReprojectC: NULL params give the defaults, max_history as a double, T the camera's inverse",
               c.run() == PTMI_OK && lookup_filled(c.a, true) && c.a.max_history == 32.0 && c.a.normal_cos == 0.9 &&
                   c.a.plane_dist == 0.02 && c.a.min_weight == 0.05);
        c.defaults = false, c.q = ptmi_reproject_params{65536, 0, 0.5, 0.25, 0.125};
        expect("ReprojectC: given params are passed on",
               c.run() == PTMI_OK && lookup_filled(c.a, true) && c.a.max_history == 65536.0 && c.a.normal_cos == 0.5 &&
                   c.a.plane_dist == 0.25 && c.a.min_weight == 0.125);
    }

    // ---- ptmi_rectify
    COMMON(RectifyC, out_hist, gathered);
    ACCEPTED(RectifyC, "out_rgba_dev NULL", c.out_rgba = 0);
    ACCEPTED(RectifyC, "out_se_dev NULL", c.out_se = 0);
    ENDS(RectifyC, radius, 1, 4);
    ENDS(RectifyC, min_count, 0, 0xffffffffu);  // (not validated)
    ENDS(RectifyC, gamma, 0.0, DBL_MAX);
    ENDS(RectifyC, max_history, 1, 65536);
    REFUSED(RectifyC, "radius 0 and 5", (c.defaults = false, c.q.radius = 0); expect("... (0)", c.run() == PTMI_ERR_ARG); c.q.radius = 5);
    {
        RectifyC c;
        expect("RectifyC: NULL params give the defaults",
               c.run() == PTMI_OK && c.a.W == (int32_t)W && c.a.H == (int32_t)H && c.a.min_count == 9 && c.a.gamma2 == 9.0 &&
                   c.a.max_history == 32.0 && c.radius == 3);
        c.defaults = false, c.q = ptmi_rectify_params{2, 5, 2.5, 7, 0};
        expect("RectifyC: gamma2 == gamma * gamma, max_history as a double, the radius beside the record",
               c.run() == PTMI_OK && c.a.gamma2 == 2.5 * 2.5 && c.a.max_history == 7.0 && c.a.min_count == 5 && c.radius == 2);
    }

    // ---- ptmi_variance_estimate
    COMMON(VarianceC, out_mom, prev_mom);
    ACCEPTED(VarianceC, "se_dev NULL", c.se = 0);
    ACCEPTED(VarianceC, "no motion table", (c.motion = 0, c.n_obj = 0));
    ACCEPTED(VarianceC, "the first frame: no moments, no records, no camera", c.no_history();
             expect("... with T = 0", c.run() == PTMI_OK && lookup_filled(c.a.r, false)));
    REFUSED(VarianceC, "out_se_dev NULL", c.out_se = 0);
    REFUSED(VarianceC, "moments without their records", c.prev_feat = 0);
    ACCEPTED(VarianceC, "out_se_dev ending where the motion table begins", c.out_se = c.motion - NPIX * 8);
    ACCEPTED(VarianceC, "out_se_dev beginning where the motion table ends", c.out_se = c.motion + 3 * PTMI_MOTION_DOUBLES * 8);
    ENDS(VarianceC, max_history, 1, 65536);
    ENDS(VarianceC, min_temporal, 2, 65536);
    ENDS(VarianceC, radius, 1, 4);
    ENDS(VarianceC, min_count, 2, 0xffffffffu);
    ENDS(VarianceC, normal_cos, 0.0, DBL_MAX);
    ENDS(VarianceC, plane_dist, 0.0, DBL_MAX);
    ENDS(VarianceC, min_weight, 0.0, DBL_MAX);
    ENDS(VarianceC, window_normal_cos, 0.0, DBL_MAX);
    REFUSED(VarianceC, "min_temporal 1 and 65537", (c.defaults = false, c.q.min_temporal = 1); expect("... (1)", c.run() == PTMI_ERR_ARG);
            c.q.min_temporal = 65537);
    REFUSED(VarianceC, "min_count 1", (c.defaults = false, c.q.min_count = 1));
    {
        VarianceC c;
        expect("VarianceC: NULL params give the defaults, T the camera's inverse",
               c.run() == PTMI_OK && lookup_filled(c.a.r, true) && c.a.r.max_history == 32.0 && c.a.r.normal_cos == 0.9 &&
                   c.a.r.plane_dist == 0.02 && c.a.r.min_weight == 0.05 && c.a.min_temporal == 4.0 &&
                   c.a.window_normal_cos == 0.9 && c.a.min_count == 9 && c.radius == 3);
        c.defaults = false, c.q = ptmi_variance_params{100, 6, 2, 4, 0, 0.5, 0.25, 0.125, 0.75};
        expect("VarianceC: given params are passed on, the counts as doubles",
               c.run() == PTMI_OK && lookup_filled(c.a.r, true) && c.a.r.max_history == 100.0 && c.a.r.normal_cos == 0.5 &&
                   c.a.r.plane_dist == 0.25 && c.a.r.min_weight == 0.125 && c.a.min_temporal == 6.0 &&
                   c.a.window_normal_cos == 0.75 && c.a.min_count == 4 && c.radius == 2);
    }
    return failures ? 1 : 0;
}
