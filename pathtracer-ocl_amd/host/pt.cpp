// pt.cpp -- Go-free counterpart of the reference CLI (cmd/pt/main.go): builds a
// named scene natively (libptmi_host.so), renders it through the drop-in
// boundary ptmi_trace (libptmi.so, MI355X) and writes the PNG the reference
// writes (tracer/pathtracer.go:17-38, "out-<samples>-<W>x<H>.png").
//
// Flags as cmd/pt/main.go:47-56 (same names and defaults):
//   --width 640 --height 480 --samples 1 --aperture 0 --focal-length 0
//   --scene gopher --device-index 0 --list-devices --list-scenes
// plus: --assets DIR (OBJ/MTL directory, default ./assets as the reference reads
// them), --out FILE.png, --raw FILE.raw (raw/writer.go format), --gpus N and
// --split sample|tile (ptmi_trace_multi over devices 0..N-1), --seed N
// (per-pixel seeds from a fixed stream; default: time-seeded like Go's
// rand.Float64 per pixel, ocltracer.go:260-263).
// Noise target (one GPU): --noise-target X renders batches of --batch B samples (default 64) of
// the --samples-spp frame through the resident-scene API (ptmi_scene_render_moments,
// ptmi_accumulate, ptmi_error_map) and stops after the first batch whose relative noise -- rms
// standard error of the pixel means over the mean pixel value -- is at most X, or when the samples
// run out; it prints samples_done and the final relative error.  --error-map FILE writes the
// standard-error map as a .raw image (one channel replicated to R, G, B).
// --adaptive (with --noise-target): every 8x8 tile stops on its own, once its rms standard error is
// at most X times the frame's mean pixel value of that batch (ptmi/error.py render_adaptive in C:
// ptmi_scene_render_tiles, ptmi_select_tiles, ptmi_finalize_counts); samples_done is then the
// largest per-tile count, and a second line gives the mean samples per pixel and the tiles that
// ran to --samples.  --sample-map FILE writes the per-pixel sample counts as a .raw image.
// --denoise (one GPU) filters the frame before the PNG / raw writers (ptmi_scene_features, ptmi_denoise
// with the library's default parameters; --denoise-iters N sets the number of a-trous passes, 1..8).
// Alone it renders every sample with moments, in batches of --batch; with --noise-target or --adaptive
// it filters the frame those loops stop at, and --error-map then holds the filtered standard error.
// --features FILE writes the first-hit normals as a .raw image (RGB = n * 0.5 + 0.5).
// --guides first|specular (default first) picks the guide records of --denoise, --temporal, --rectify and
// --features: the first hits, or the first surface behind mirrors and glass at its virtual position
// (ptmi_scene_features_chain; --max-chain N, 1..16, default 8, bounds the chain).  Not with --move-object.
// --frames N (N > 1, one GPU) renders N views from one resident scene (ptmi_scene_set_camera): frame k's
// camera is the scene's turned by k x --orbit-step degrees about the world y axis (ptmi/temporal.py
// orbit_camera: inverse' = rotate_y * inverse, Go's Sin and Cos), its seeds come from --seed + k, and its
// PNG takes the frame number before the extension (turn.png -> turn.0000.png, ...).  --temporal
// accumulates across the frames (ptmi_reproject; --max-history N, default 32); --denoise then filters
// the accumulated frame.  --move-object I --move-step DX,DY,DZ moves object I of the scene's list along the
// sequence (ptmi_scene_set_objects): in frame k it carries translate(k * step) * transform with the inverse and
// inverse transpose of that product (ptmi/temporal.py move_object), and --temporal then follows it
// (ptmi_motion_table, ptmi_reproject_motion).  --rectify (with --temporal) tests the history against each
// frame before it is blended (ptmi_history_gather, ptmi_rectify; --rectify-gamma G, default 3, and
// --rectify-radius R, 1..4, default 3), and --emission-step F multiplies the emission of every emissive object
// by F from frame N / 2 on (ptmi_scene_set_objects): a lighting change from the command line.
// --estimate-variance (with --temporal) estimates each frame's standard error from the moments of each surface
// point's frames and, where that history is short, from a window of same-surface pixels (ptmi_variance_estimate on
// a moment history of its own; --var-min-history N, 2..65536, default 4, and --var-radius R, 1..4, default 3), and
// the accumulation, --rectify and --denoise take that map in the place of the rendered one: --samples 1 is then a
// normal input.
// An unknown --scene renders the OCL scene, as main.go:86-88 does.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/ptmi.h"
#include "../../include/ptmi_host.h"
#include "geom.h"

namespace {

struct Cfg {
    int width = 640, height = 480, samples = 1, device_index = 0;
    double aperture = 0.0, focal_length = 0.0;
    std::string scene = "gopher", assets = "assets", out, raw, split = "sample";
    int gpus = 1;
    bool list_devices = false, list_scenes = false, have_seed = false;
    uint64_t seed = 0;
    bool have_target = false;
    double noise_target = 0.0;
    int batch = 64;
    std::string error_map;
    bool adaptive = false;
    std::string sample_map;
    bool denoise = false, have_iters = false;
    int denoise_iters = 0;  // 0: the library's default
    std::string features;
    int frames = 1, max_history = 0;  // 0: the library's default
    bool have_frames = false, have_step = false, temporal = false;
    double orbit_step = 0.0;
    int move_object = -1;
    bool have_move = false, have_move_step = false;
    double move_step[3] = {0.0, 0.0, 0.0};
    bool rectify = false, have_gamma = false, have_radius = false, have_emission = false;
    double rectify_gamma = 3.0, emission_step = 1.0;
    int rectify_radius = 3;
    std::string guides = "first";
    int max_chain = 8;
    bool have_guides = false, have_chain = false;
    bool estimate_variance = false, have_var_history = false, have_var_radius = false;
    int var_min_history = 4, var_radius = 3;
};

// The guide records of the scene's camera: the first hits, or with --guides specular the chains' final surfaces.
int trace_guides(const Cfg& c, ptmi_scene* sc, double* feat, char* err, size_t err_len) {
    if (c.guides == "specular") return ptmi_scene_features_chain(sc, feat, (uint32_t)c.max_chain, 0.5, nullptr, err, err_len);
    return ptmi_scene_features(sc, feat, nullptr, err, err_len);
}

[[noreturn]] void usage(const char* msg) {
    std::fprintf(stderr,
                 "%s\nusage: pt [--width N] [--height N] [--samples N] [--aperture F] [--focal-length F]\n"
                 "          [--scene NAME] [--device-index N] [--list-devices] [--list-scenes]\n"
                 "          [--assets DIR] [--out FILE.png] [--raw FILE.raw] [--gpus N] [--split sample|tile]\n"
                 "          [--seed N] [--noise-target X] [--batch N] [--error-map FILE.raw]\n"
                 "          [--adaptive] [--sample-map FILE.raw] [--denoise] [--denoise-iters N]\n"
                 "          [--features FILE.raw] [--frames N] [--orbit-step DEGREES] [--temporal] [--max-history N]\n"
                 "          [--move-object I --move-step DX,DY,DZ] [--rectify] [--rectify-gamma G] [--rectify-radius R]\n"
                 "          [--emission-step F] [--guides first|specular] [--max-chain N]\n"
                 "          [--estimate-variance] [--var-min-history N] [--var-radius R]\n",
                 msg);
    std::exit(2);
}

Cfg parse(int argc, char** argv) {
    Cfg c;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], v;
        const size_t eq = a.find('=');
        bool inl = false;
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
            v = a.substr(eq + 1);
            a = a.substr(0, eq);
            inl = true;
        }
        auto val = [&]() -> std::string {
            if (inl) return v;
            if (i + 1 >= argc) usage(("missing value for " + a).c_str());
            return argv[++i];
        };
        if (a == "--width") c.width = std::atoi(val().c_str());
        else if (a == "--height") c.height = std::atoi(val().c_str());
        else if (a == "--samples") c.samples = std::atoi(val().c_str());
        else if (a == "--aperture") c.aperture = std::atof(val().c_str());
        else if (a == "--focal-length") c.focal_length = std::atof(val().c_str());
        else if (a == "--scene") c.scene = val();
        else if (a == "--device-index") c.device_index = std::atoi(val().c_str());
        else if (a == "--list-devices") c.list_devices = true;
        else if (a == "--list-scenes") c.list_scenes = true;
        else if (a == "--assets") c.assets = val();
        else if (a == "--out") c.out = val();
        else if (a == "--raw") c.raw = val();
        else if (a == "--gpus") c.gpus = std::atoi(val().c_str());
        else if (a == "--split") c.split = val();
        else if (a == "--seed") c.seed = std::strtoull(val().c_str(), nullptr, 10), c.have_seed = true;
        else if (a == "--noise-target") c.noise_target = std::atof(val().c_str()), c.have_target = true;
        else if (a == "--batch") c.batch = std::atoi(val().c_str());
        else if (a == "--error-map") c.error_map = val();
        else if (a == "--adaptive") c.adaptive = true;
        else if (a == "--sample-map") c.sample_map = val();
        else if (a == "--denoise") c.denoise = true;
        else if (a == "--denoise-iters") c.denoise_iters = std::atoi(val().c_str()), c.have_iters = true;
        else if (a == "--features") c.features = val();
        else if (a == "--frames") c.frames = std::atoi(val().c_str()), c.have_frames = true;
        else if (a == "--orbit-step") c.orbit_step = std::atof(val().c_str()), c.have_step = true;
        else if (a == "--temporal") c.temporal = true;
        else if (a == "--move-object") c.move_object = std::atoi(val().c_str()), c.have_move = true;
        else if (a == "--move-step") {
            if (std::sscanf(val().c_str(), "%lf,%lf,%lf", &c.move_step[0], &c.move_step[1], &c.move_step[2]) != 3)
                usage("--move-step takes DX,DY,DZ");
            c.have_move_step = true;
        }
        else if (a == "--max-history") c.max_history = std::atoi(val().c_str());
        else if (a == "--rectify") c.rectify = true;
        else if (a == "--rectify-gamma") c.rectify_gamma = std::atof(val().c_str()), c.have_gamma = true;
        else if (a == "--rectify-radius") c.rectify_radius = std::atoi(val().c_str()), c.have_radius = true;
        else if (a == "--emission-step") c.emission_step = std::atof(val().c_str()), c.have_emission = true;
        else if (a == "--guides") c.guides = val(), c.have_guides = true;
        else if (a == "--max-chain") c.max_chain = std::atoi(val().c_str()), c.have_chain = true;
        else if (a == "--estimate-variance") c.estimate_variance = true;
        else if (a == "--var-min-history") c.var_min_history = std::atoi(val().c_str()), c.have_var_history = true;
        else if (a == "--var-radius") c.var_radius = std::atoi(val().c_str()), c.have_var_radius = true;
        else if (a == "--help" || a == "-h") usage("pt: path tracer on AMD Instinct GPUs");
        else usage(("unknown flag " + a).c_str());
    }
    if (c.width <= 0 || c.height <= 0 || c.samples <= 0) usage("width, height and samples must be positive");
    if (c.gpus <= 0 || (c.split != "sample" && c.split != "tile")) usage("--gpus must be >= 1, --split sample|tile");
    if ((c.have_target || !c.error_map.empty()) && c.gpus > 1)
        usage("--noise-target and --error-map need --gpus 1");
    if ((c.adaptive || !c.sample_map.empty()) && c.gpus > 1) usage("--adaptive and --sample-map need --gpus 1");
    if (c.have_iters && !c.denoise) usage("--denoise-iters needs --denoise");
    if ((c.denoise || !c.features.empty()) && c.gpus > 1) usage("--denoise and --features need --gpus 1");
    if (c.have_iters && (c.denoise_iters < 1 || c.denoise_iters > 8)) usage("--denoise-iters must be 1..8");
    if (c.adaptive && !c.have_target) usage("--adaptive needs --noise-target");
    if (!c.sample_map.empty() && !c.adaptive) usage("--sample-map needs --adaptive");
    if (c.adaptive && c.batch < 2) usage("--adaptive needs --batch >= 2");
    if (c.have_frames && c.frames < 1) usage("--frames must be >= 1");
    const bool sequence = c.frames > 1;
    if (c.temporal && !sequence) usage("--temporal needs --frames N with N > 1");
    if ((c.temporal || sequence) && (c.gpus > 1 || c.adaptive || c.have_target))
        usage("--frames and --temporal need --gpus 1 and take neither --adaptive nor --noise-target");
    if (sequence && (!c.raw.empty() || !c.error_map.empty() || !c.features.empty()))
        usage("--frames writes PNG frames only (no --raw, --error-map or --features)");
    if (c.have_step && !sequence) usage("--orbit-step needs --frames N with N > 1");
    if ((c.have_move || c.have_move_step) && !sequence) usage("--move-object and --move-step need --frames N with N > 1");
    if (c.have_move != c.have_move_step) usage("--move-object I and --move-step DX,DY,DZ go together");
    if (c.have_move && c.move_object < 0) usage("--move-object must be an index into the scene's objects");
    if (c.max_history && !c.temporal) usage("--max-history needs --temporal");
    if (c.temporal && c.max_history && (c.max_history < 1 || c.max_history > 65536)) usage("--max-history must be 1..65536");
    if (c.max_history < 0) usage("--max-history must be 1..65536");
    if (c.rectify && !c.temporal) usage("--rectify needs --temporal");
    if ((c.have_gamma || c.have_radius) && !c.rectify) usage("--rectify-gamma and --rectify-radius need --rectify");
    if (c.have_gamma && !(std::isfinite(c.rectify_gamma) && c.rectify_gamma >= 0.0)) usage("--rectify-gamma must be finite and >= 0");
    if (c.have_radius && (c.rectify_radius < 1 || c.rectify_radius > 4)) usage("--rectify-radius must be 1..4");
    if (c.have_emission && !sequence) usage("--emission-step needs --frames N with N > 1");
    if (c.have_emission && !(std::isfinite(c.emission_step) && c.emission_step >= 0.0)) usage("--emission-step must be finite and >= 0");
    if (c.estimate_variance && !c.temporal) usage("--estimate-variance needs --temporal");
    if ((c.have_var_history || c.have_var_radius) && !c.estimate_variance)
        usage("--var-min-history and --var-radius need --estimate-variance");
    if (c.have_var_history && (c.var_min_history < 2 || c.var_min_history > 65536)) usage("--var-min-history must be 2..65536");
    if (c.have_var_radius && (c.var_radius < 1 || c.var_radius > 4)) usage("--var-radius must be 1..4");
    if (c.temporal && c.samples < 2 && !c.estimate_variance)
        usage("--temporal needs --samples >= 2 (the variance of a frame)");
    if (c.guides != "first" && c.guides != "specular") usage("--guides first|specular");
    if (c.have_guides && !(c.denoise || c.temporal || !c.features.empty()))
        usage("--guides needs --denoise, --temporal or --features");
    if (c.have_chain && c.guides != "specular") usage("--max-chain needs --guides specular");
    if (c.have_chain && (c.max_chain < 1 || c.max_chain > 16)) usage("--max-chain must be 1..16");
    if (c.guides == "specular" && c.have_move) usage("--guides specular does not follow --move-object");
    if (c.batch <= 0 || (c.have_target && !(c.noise_target >= 0.0))) usage("--batch must be positive, --noise-target >= 0");
    return c;
}

// The noise-target loop (ptmi/error.py render_to_noise in C): batches [k * batch, (k + 1) * batch) of
// the samples-spp frame until stats[0] <= target * stats[2].  Without a target (--error-map alone)
// it renders every sample.  out: RGBA of the samples done; se: the standard-error map as RGBA.
// --adaptive: each batch runs on the tiles still above the threshold (two lists, ping-pong), and the
// frame is finalised by each pixel's own count; counts_rgba: the counts as RGBA, tiles_at_max: the
// tiles that took every sample.
int render_noise(const Cfg& c, const ptmi_records& r, const ptmi_textures* tex, uint64_t stream_seed,
                 std::vector<double>& out, std::vector<double>& se_rgba, uint32_t& done, double& rel,
                 std::vector<double>& counts_rgba, uint32_t& tiles_at_max, std::vector<double>& normals_rgba, char* err,
                 size_t err_len) {
    const size_t n = (size_t)c.width * c.height;
    const uint32_t tiles = (uint32_t)((c.width + 7) / 8) * (uint32_t)((c.height + 7) / 8);
    ptmi_scene* sc = nullptr;
    double *seeds = nullptr, *sums = nullptr, *sq = nullptr, *b_sums = nullptr, *b_sq = nullptr, *se = nullptr,
           *stats = nullptr, *tile_err = nullptr;
    uint32_t* lists = nullptr;  // adaptive: two tile lists and the selected count behind them
    double *feat = nullptr, *dn_out = nullptr, *dn_se = nullptr, *dn_work = nullptr;  // --denoise / --features
    tiles_at_max = 0;
    int rc = ptmi_scene_create_textured(c.device_index, r.objects, r.n_obj, r.triangles, r.n_tri, r.groups, r.n_grp,
                                        r.camera, tex, &sc, err, err_len);
    if (rc) return rc;
    auto hip = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return false;
        std::snprintf(err, err_len, "%s failed: %s", what, hipGetErrorString(e));
        rc = PTMI_ERR_HIP;
        return true;
    };
    const uint32_t samples = (uint32_t)c.samples;
    std::vector<double> se_host(n);
    double st[4] = {0, 0, 0, 0};
    done = 0;
    rel = 0.0;
    // The finished frame (image: RGBA, se: the standard-error map, both on the device) to the host,
    // through the feature pass and the filter when they are asked for.
    auto finish = [&](const double* image) -> bool {
        const double* se_final = se;
        if (c.denoise || !c.features.empty()) {
            if (hip(hipMalloc((void**)&feat, n * PTMI_FEATURE_DOUBLES * sizeof(double)), "hipMalloc")) return false;
            if ((rc = trace_guides(c, sc, feat, err, err_len))) return false;
        }
        if (!c.features.empty()) {
            std::vector<double> fh(n * PTMI_FEATURE_DOUBLES);
            if (hip(hipMemcpy(fh.data(), feat, fh.size() * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy"))
                return false;
            normals_rgba.resize(n * 4);
            for (size_t i = 0; i < n; i++) {
                for (int k = 0; k < 3; k++) normals_rgba[4 * i + k] = fh[PTMI_FEATURE_DOUBLES * i + 4 + k] * 0.5 + 0.5;
                normals_rgba[4 * i + 3] = 1.0;
            }
        }
        if (c.denoise) {
            const size_t wb = ptmi_denoise_work_bytes((uint32_t)c.width, (uint32_t)c.height);
            if (hip(hipMalloc((void**)&dn_out, n * 4 * sizeof(double)), "hipMalloc")) return false;
            if (hip(hipMalloc((void**)&dn_se, n * sizeof(double)), "hipMalloc")) return false;
            if (hip(hipMalloc((void**)&dn_work, wb), "hipMalloc")) return false;
            ptmi_denoise_params dp{5, PTMI_DENOISE_DEMODULATE, 4.0, 0.01, 7, 0};
            if (c.denoise_iters) dp.iterations = (uint32_t)c.denoise_iters;
            if ((rc = ptmi_denoise(image, se, feat, (uint32_t)c.width, (uint32_t)c.height, &dp, dn_out, dn_se, dn_work,
                                   wb, nullptr, err, err_len)))
                return false;
            image = dn_out;
            se_final = dn_se;
        }
        if (hip(hipMemcpy(out.data(), image, n * 4 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy")) return false;
        if (hip(hipMemcpy(se_host.data(), se_final, n * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy")) return false;
        return true;
    };
    do {
        if (hip(hipSetDevice(c.device_index), "hipSetDevice")) break;
        if (hip(hipMalloc((void**)&seeds, n * sizeof(double)), "hipMalloc")) break;
        if (hip(hipMalloc((void**)&sums, n * 4 * sizeof(double)), "hipMalloc")) break;
        if (hip(hipMalloc((void**)&sq, n * sizeof(double)), "hipMalloc")) break;
        if (hip(hipMalloc((void**)&b_sums, n * 4 * sizeof(double)), "hipMalloc")) break;
        if (hip(hipMalloc((void**)&b_sq, n * sizeof(double)), "hipMalloc")) break;
        if (hip(hipMalloc((void**)&se, n * sizeof(double)), "hipMalloc")) break;
        if (hip(hipMalloc((void**)&stats, 4 * sizeof(double)), "hipMalloc")) break;
        if (hip(hipMemset(sums, 0, n * 4 * sizeof(double)), "hipMemset")) break;
        if (hip(hipMemset(sq, 0, n * sizeof(double)), "hipMemset")) break;
        if ((rc = ptmi_fill_seeds(seeds, (uint32_t)n, stream_seed, nullptr, err, err_len))) break;
        if (c.adaptive) {
            if (hip(hipMalloc((void**)&tile_err, tiles * sizeof(double)), "hipMalloc")) break;
            if (hip(hipMalloc((void**)&lists, ((size_t)2 * tiles + 1) * sizeof(uint32_t)), "hipMalloc")) break;
            std::vector<uint32_t> all(tiles);
            for (uint32_t t = 0; t < tiles; t++) all[t] = t;
            if (hip(hipMemcpy(lists, all.data(), tiles * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy")) break;
            uint32_t *cur = lists, *nxt = lists + tiles, *count = lists + 2 * (size_t)tiles, active = tiles;
            while (true) {
                const uint32_t end = std::min<uint64_t>((uint64_t)done + (uint32_t)c.batch, samples);
                if ((rc = ptmi_scene_render_tiles(sc, samples, done, end, cur, active, seeds, b_sums, b_sq, 0, nullptr,
                                                  err, err_len)))
                    break;
                if ((rc = ptmi_accumulate(sums, b_sums, n * 4, nullptr, err, err_len))) break;
                if ((rc = ptmi_accumulate(sq, b_sq, n, nullptr, err, err_len))) break;
                if ((rc = ptmi_error_map(sums, sq, (uint32_t)c.width, (uint32_t)c.height, se, tile_err, stats, nullptr,
                                         err, err_len)))
                    break;
                if (hip(hipMemcpy(st, stats, sizeof(st), hipMemcpyDeviceToHost), "hipMemcpy")) break;
                done = end;
                rel = st[2] != 0.0 ? st[0] / st[2] : HUGE_VAL;
                if (done == samples) tiles_at_max = active;
                if ((rc = ptmi_select_tiles(tile_err, cur, active, c.noise_target * st[2], nxt, count, nullptr, err,
                                            err_len)))
                    break;
                if (hip(hipMemcpy(&active, count, sizeof(active), hipMemcpyDeviceToHost), "hipMemcpy")) break;
                std::swap(cur, nxt);
                if (active == 0 || done == samples) break;
            }
            if (rc) break;
            if ((rc = ptmi_finalize_counts(sums, b_sums, (uint32_t)n, nullptr, err, err_len))) break;
            counts_rgba.resize(n * 4);
            if (hip(hipMemcpy(counts_rgba.data(), sums, n * 4 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy"))
                break;
            for (size_t i = 0; i < n; i++) {
                counts_rgba[4 * i + 0] = counts_rgba[4 * i + 1] = counts_rgba[4 * i + 2] = counts_rgba[4 * i + 3];
                counts_rgba[4 * i + 3] = 1.0;
            }
            (void)finish(b_sums);
            break;
        }
        while (done < samples) {
            const uint32_t end = std::min<uint64_t>((uint64_t)done + (uint32_t)c.batch, samples);
            if ((rc = ptmi_scene_render_moments(sc, samples, done, end, 1, 0, seeds, b_sums, b_sq, 0, nullptr, err,
                                                err_len)))
                break;
            if ((rc = ptmi_accumulate(sums, b_sums, n * 4, nullptr, err, err_len))) break;
            if ((rc = ptmi_accumulate(sq, b_sq, n, nullptr, err, err_len))) break;
            if ((rc = ptmi_error_map(sums, sq, (uint32_t)c.width, (uint32_t)c.height, se, nullptr, stats, nullptr, err,
                                     err_len)))
                break;
            if (hip(hipMemcpy(st, stats, sizeof(st), hipMemcpyDeviceToHost), "hipMemcpy")) break;
            done = end;
            rel = st[2] != 0.0 ? st[0] / st[2] : HUGE_VAL;
            if (c.have_target && st[0] <= c.noise_target * st[2]) break;
        }
        if (rc) break;
        if ((rc = ptmi_finalize(sums, sums, (uint32_t)n, done, nullptr, err, err_len))) break;
        (void)finish(sums);
    } while (false);
    for (double* p : {seeds, sums, sq, b_sums, b_sq, se, stats, tile_err, feat, dn_out, dn_se, dn_work})
        if (p) (void)hipFree(p);
    if (lists) (void)hipFree(lists);
    ptmi_scene_destroy(sc);
    se_rgba.resize(n * 4);
    for (size_t i = 0; i < n; i++) {
        se_rgba[4 * i + 0] = se_rgba[4 * i + 1] = se_rgba[4 * i + 2] = se_host[i];
        se_rgba[4 * i + 3] = 1.0;
    }
    return rc;
}

// "turn.png" -> "turn.0007.png"
std::string frame_name(const std::string& png, int k) {
    char num[16];
    std::snprintf(num, sizeof(num), ".%04d", k);
    const size_t dot = png.rfind('.'), slash = png.rfind('/');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return png + num;
    return png.substr(0, dot) + num + png.substr(dot);
}

// --frames: N views of one resident scene (ptmi/temporal.py render_sequence in C).  Per frame k:
// ptmi_scene_set_camera(the camera turned by k * orbit_step), seeds from stream_seed + k, a moment render
// of every sample, the error map, finalize, and -- with --temporal or --denoise -- the feature pass, the
// accumulation against frame k - 1 (history and records ping-pong) and the filter.  One PNG per frame.
int render_frames(const Cfg& c, const ptmi_records& r, const ptmi_textures* tex, uint64_t stream_seed,
                  const std::string& png, char* err, size_t err_len) {
    const size_t n = (size_t)c.width * c.height;
    const uint32_t W = (uint32_t)c.width, H = (uint32_t)c.height, samples = (uint32_t)c.samples;
    ptmi_scene* sc = nullptr;
    int rc = ptmi_scene_create_textured(c.device_index, r.objects, r.n_obj, r.triangles, r.n_tri, r.groups, r.n_grp,
                                        r.camera, tex, &sc, err, err_len);
    if (rc) return rc;
    double *seeds = nullptr, *sums = nullptr, *sq = nullptr, *se = nullptr, *stats = nullptr, *image = nullptr,
           *acc = nullptr, *acc_se = nullptr, *dn_out = nullptr, *dn_se = nullptr, *dn_work = nullptr, *motion = nullptr,
           *gathered = nullptr, *se_est = nullptr;
    double *feat[2] = {nullptr, nullptr}, *hist[2] = {nullptr, nullptr}, *mom[2] = {nullptr, nullptr};
    auto hip = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return false;
        std::snprintf(err, err_len, "%s failed: %s", what, hipGetErrorString(e));
        rc = PTMI_ERR_HIP;
        return true;
    };
    auto dmalloc = [&](double** p, size_t doubles) { return hip(hipMalloc((void**)p, doubles * sizeof(double)), "hipMalloc"); };
    const bool guides = c.temporal || c.denoise;
    const size_t wb = ptmi_denoise_work_bytes(W, H);
    std::vector<double> out(n * 4);
    unsigned char cam0[PTMI_CAMERA_BYTES], cam[PTMI_CAMERA_BYTES], prev_cam[PTMI_CAMERA_BYTES];
    std::memcpy(cam0, r.camera, sizeof(cam0));
    ptmi_host::Mat inv0;
    std::memcpy(inv0.data(), cam0 + 56, sizeof(double) * 16);  // CLCamera.inverse (ocltracer.go:85-96)
    // --move-object: the frame's object records (the moved object's three matrices replaced) and the previous frame's
    const bool moving = c.have_move;
    const size_t obj_bytes = (size_t)r.n_obj * PTMI_OBJECT_BYTES;
    std::vector<unsigned char> objs, prev_objs;
    ptmi_host::Mat transform0 = ptmi_host::identity();
    if (moving || c.have_emission) {
        objs.assign((const unsigned char*)r.objects, (const unsigned char*)r.objects + obj_bytes);
        if (moving) std::memcpy(transform0.data(), objs.data() + (size_t)c.move_object * PTMI_OBJECT_BYTES, sizeof(double) * 16);
    }
    do {
        if (hip(hipSetDevice(c.device_index), "hipSetDevice")) break;
        if (dmalloc(&seeds, n) || dmalloc(&sums, n * 4) || dmalloc(&sq, n) || dmalloc(&se, n) || dmalloc(&stats, 4) ||
            dmalloc(&image, n * 4))
            break;
        if (guides && (dmalloc(&feat[0], n * PTMI_FEATURE_DOUBLES) || dmalloc(&feat[1], n * PTMI_FEATURE_DOUBLES))) break;
        if (c.temporal && (dmalloc(&hist[0], n * PTMI_HISTORY_DOUBLES) || dmalloc(&hist[1], n * PTMI_HISTORY_DOUBLES) ||
                           dmalloc(&acc, n * 4) || dmalloc(&acc_se, n)))
            break;
        if (c.denoise && (dmalloc(&dn_out, n * 4) || dmalloc(&dn_se, n) || hip(hipMalloc((void**)&dn_work, wb), "hipMalloc")))
            break;
        if (moving && c.temporal && dmalloc(&motion, (size_t)PTMI_MOTION_DOUBLES * PTMI_MAX_OBJECTS)) break;
        if (c.rectify && dmalloc(&gathered, n * PTMI_HISTORY_DOUBLES)) break;
        if (c.estimate_variance &&
            (dmalloc(&mom[0], n * PTMI_MOMENT_DOUBLES) || dmalloc(&mom[1], n * PTMI_MOMENT_DOUBLES) || dmalloc(&se_est, n)))
            break;
        for (int k = 0; k < c.frames && !rc; k++) {
            if (moving) {
                prev_objs = objs;
                const ptmi_host::Mat t = ptmi_host::multiply(
                    ptmi_host::translate((double)k * c.move_step[0], (double)k * c.move_step[1], (double)k * c.move_step[2]),
                    transform0);
                const ptmi_host::Mat ti = ptmi_host::inverse(t), tit = ptmi_host::transpose(ti);
                unsigned char* o = objs.data() + (size_t)c.move_object * PTMI_OBJECT_BYTES;
                std::memcpy(o, t.data(), 128);  // CLObject.transform, inverse, inverseTranspose (ocltracer.go:25-28)
                std::memcpy(o + 128, ti.data(), 128);
                std::memcpy(o + 256, tit.data(), 128);
            }
            const bool dim = c.have_emission && k == c.frames / 2;
            if (dim) {  // CLObject.emission (ocltracer.go:25-28): rgb of every object, times F (0 stays 0)
                for (uint32_t j = 0; j < r.n_obj; j++) {
                    double e[3];
                    unsigned char* o = objs.data() + (size_t)j * PTMI_OBJECT_BYTES + 416;
                    std::memcpy(e, o, sizeof(e));
                    for (double& v : e) v = v * c.emission_step;
                    std::memcpy(o, e, sizeof(e));
                }
            }
            if ((moving || dim) && (rc = ptmi_scene_set_objects(sc, objs.data(), r.n_obj, err, err_len))) break;
            std::memcpy(cam, cam0, sizeof(cam));
            const ptmi_host::Mat rot = ptmi_host::rotate_y(((double)k * c.orbit_step) * M_PI / 180.0);
            const ptmi_host::Mat inv = ptmi_host::multiply(rot, inv0);
            std::memcpy(cam + 56, inv.data(), sizeof(double) * 16);
            if ((rc = ptmi_scene_set_camera(sc, cam, err, err_len))) break;
            if ((rc = ptmi_fill_seeds(seeds, (uint32_t)n, stream_seed + (uint64_t)k, nullptr, err, err_len))) break;
            if ((rc = ptmi_scene_render_moments(sc, samples, 0, samples, 1, 0, seeds, sums, sq, 0, nullptr, err, err_len)))
                break;
            if ((rc = ptmi_error_map(sums, sq, W, H, se, nullptr, stats, nullptr, err, err_len))) break;
            if ((rc = ptmi_finalize(sums, image, (uint32_t)n, samples, nullptr, err, err_len))) break;
            const double *frame = image, *frame_se = se;
            double* f = feat[k & 1];
            if (guides && (rc = trace_guides(c, sc, f, err, err_len))) break;
            if (c.temporal) {
                ptmi_reproject_params rp{32, 0, 0.9, 0.02, 0.05};
                if (c.max_history) rp.max_history = (uint32_t)c.max_history;
                if (moving && k && (rc = ptmi_motion_table(prev_objs.data(), objs.data(), r.n_obj, motion, nullptr, err, err_len)))
                    break;
                const double* se_in = se;  // the standard error the accumulation and the filter take
                if (c.estimate_variance) {
                    ptmi_variance_params vp{rp.max_history, (uint32_t)c.var_min_history, (uint32_t)c.var_radius, 9, 0,
                                            rp.normal_cos, rp.plane_dist, rp.min_weight, 0.9};
                    if ((rc = ptmi_variance_estimate(image, se, f, k ? mom[(k - 1) & 1] : nullptr, k ? feat[(k - 1) & 1] : nullptr,
                                                     k ? prev_cam : nullptr, W, H, &vp, mom[k & 1], se_est,
                                                     moving && k ? motion : nullptr, moving && k ? r.n_obj : 0, nullptr, err,
                                                     err_len)))
                        break;
                    se_in = se_est;
                }
                if (c.rectify) {
                    ptmi_rectify_params tp{(uint32_t)c.rectify_radius, 9, c.rectify_gamma, rp.max_history, 0};
                    if ((rc = ptmi_history_gather(image, se_in, f, k ? hist[(k - 1) & 1] : nullptr, k ? feat[(k - 1) & 1] : nullptr,
                                                  k ? prev_cam : nullptr, W, H, &rp, gathered, moving && k ? motion : nullptr,
                                                  moving && k ? r.n_obj : 0, nullptr, err, err_len)))
                        break;
                    rc = ptmi_rectify(image, se_in, f, gathered, W, H, &tp, hist[k & 1], acc, acc_se, nullptr, err, err_len);
                } else if (moving && k) {
                    rc = ptmi_reproject_motion(image, se_in, f, hist[(k - 1) & 1], feat[(k - 1) & 1], prev_cam, W, H, &rp,
                                               hist[k & 1], acc, acc_se, motion, r.n_obj, nullptr, err, err_len);
                } else {
                    rc = ptmi_reproject(image, se_in, f, k ? hist[(k - 1) & 1] : nullptr, k ? feat[(k - 1) & 1] : nullptr,
                                        k ? prev_cam : nullptr, W, H, &rp, hist[k & 1], acc, acc_se, nullptr, err, err_len);
                }
                if (rc) break;
                frame = acc;
                frame_se = acc_se;
            }
            if (c.denoise) {
                ptmi_denoise_params dp{5, PTMI_DENOISE_DEMODULATE, 4.0, 0.01, 7, 0};
                if (c.denoise_iters) dp.iterations = (uint32_t)c.denoise_iters;
                if ((rc = ptmi_denoise(frame, frame_se, f, W, H, &dp, dn_out, dn_se, dn_work, wb, nullptr, err, err_len)))
                    break;
                frame = dn_out;
            }
            if (hip(hipMemcpy(out.data(), frame, n * 4 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy")) break;
            std::memcpy(prev_cam, cam, sizeof(cam));
            const std::string name = frame_name(png, k);
            if ((rc = ptmi_host_write_png(name.c_str(), out.data(), c.width, c.height, err, err_len))) break;
            std::fprintf(stderr, "frame %d (%.6g degrees): wrote %s\n", k, (double)k * c.orbit_step, name.c_str());
        }
    } while (false);
    for (double* p : {seeds, sums, sq, se, stats, image, acc, acc_se, dn_out, dn_se, dn_work, motion, gathered, se_est, feat[0],
                      feat[1], hist[0], hist[1], mom[0], mom[1]})
        if (p) (void)hipFree(p);
    ptmi_scene_destroy(sc);
    return rc;
}

bool known_scene(const std::string& s) {
    const std::string names = ptmi_host_scene_names();
    size_t a = 0;
    while (a < names.size()) {
        const size_t b = names.find('\n', a);
        if (names.compare(a, b - a, s) == 0 && b - a == s.size()) return true;
        a = b + 1;
    }
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    const Cfg c = parse(argc, argv);
    char err[512] = {0};
    if (c.list_devices) {  // main.go:98-112
        const int n = ptmi_device_count();
        for (int i = 0; i < n; i++) {
            char name[256];
            if (ptmi_device_name(i, name, sizeof(name)) == PTMI_OK)
                std::printf("Index: %d Type: GPU Name: %s\n", i, name);
        }
        return 0;
    }
    if (c.list_scenes) {
        std::fputs(ptmi_host_scene_names(), stdout);
        return 0;
    }
    const std::string scene = known_scene(c.scene) ? c.scene : "default";
    const auto t0 = std::chrono::steady_clock::now();
    ptmi_records r;
    int rc = ptmi_host_build_scene(scene.c_str(), c.width, c.height, c.aperture, c.focal_length, c.assets.c_str(),
                                   &r, err, sizeof(err));
    if (rc) {
        std::fprintf(stderr, "scene build failed (%d): %s\n", rc, err);
        return 1;
    }
    ptmi_textures tex;  // the scene's texture arrays (texturedplanets / envmap / cubemap)
    if ((rc = ptmi_host_load_scene_textures(scene.c_str(), c.assets.c_str(), &tex, err, sizeof(err)))) {
        ptmi_host_free_records(&r);
        std::fprintf(stderr, "%s\n", err);  // the reference: LoadImage panics
        return 1;
    }
    const bool textured = tex.count[0] || tex.count[1] || tex.count[2];
    const auto t1 = std::chrono::steady_clock::now();
    const size_t n = (size_t)c.width * c.height;
    std::vector<double> out(n * 4);
    const uint64_t stream =
        c.have_seed ? c.seed : (uint64_t)std::chrono::system_clock::now().time_since_epoch().count();
    ptmi_multi_timing mt{};
    const bool noise = c.have_target || !c.error_map.empty() || c.denoise || !c.features.empty();
    std::vector<double> normals_rgba;
    std::vector<double> se_rgba;
    uint32_t samples_done = (uint32_t)c.samples;
    double rel_err = 0.0;
    std::vector<double> counts_rgba;
    uint32_t tiles_at_max = 0;
    const std::string png = c.out.empty() ? "out-" + std::to_string(c.samples) + "-" + std::to_string(c.width) +
                                                     "x" + std::to_string(c.height) + ".png"
                                               : c.out;
    if (c.have_move && (uint32_t)c.move_object >= r.n_obj) {
        ptmi_host_free_records(&r);
        ptmi_host_free_textures(&tex);
        usage("--move-object is outside the scene's objects");
    }
    if (c.frames > 1) {  // a camera sequence: its frames are written as they finish
        rc = render_frames(c, r, textured ? &tex : nullptr, stream, png, err, sizeof(err));
        ptmi_host_free_records(&r);
        ptmi_host_free_textures(&tex);
        if (rc) {
            std::fprintf(stderr, "sequence render failed (%d): %s\n", rc, err);
            return 1;
        }
        const double trace_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        std::fprintf(stderr, "scene %s: %d frames of %dx%d x %d spp in %.3f s\n", scene.c_str(), c.frames, c.width,
                     c.height, c.samples, trace_s);
        return 0;
    }
    if (noise) {
        rc = render_noise(c, r, textured ? &tex : nullptr, stream, out, se_rgba, samples_done, rel_err, counts_rgba,
                          tiles_at_max, normals_rgba, err, sizeof(err));
    } else if (c.gpus == 1) {
        rc = ptmi_trace(r.objects, r.n_obj, r.triangles, r.n_tri, r.groups, r.n_grp, c.device_index,
                        (uint32_t)c.samples, r.camera, nullptr, stream, textured ? &tex : nullptr, out.data(), err,
                        sizeof(err));
    } else {
        std::vector<int> devs(c.gpus);
        for (int d = 0; d < c.gpus; d++) devs[d] = d;
        rc = ptmi_trace_multi_timed(r.objects, r.n_obj, r.triangles, r.n_tri, r.groups, r.n_grp, devs.data(),
                                    (uint32_t)c.gpus, c.split == "tile" ? 1 : 0, (uint32_t)c.samples, r.camera,
                                    nullptr, stream, textured ? &tex : nullptr, out.data(), &mt, err, sizeof(err));
    }
    ptmi_host_free_records(&r);
    ptmi_host_free_textures(&tex);
    if (rc) {
        std::fprintf(stderr, "ptmi_trace failed (%d): %s\n", rc, err);  // the reference: logrus.Fatalf
        return 1;
    }
    const auto t2 = std::chrono::steady_clock::now();
    if ((rc = ptmi_host_write_png(png.c_str(), out.data(), c.width, c.height, err, sizeof(err)))) {
        std::fprintf(stderr, "%s\n", err);
        return 1;
    }
    if (!c.raw.empty() && (rc = ptmi_host_write_raw(c.raw.c_str(), out.data(), c.width, c.height, err, sizeof(err)))) {
        std::fprintf(stderr, "%s\n", err);
        return 1;
    }
    if (!c.error_map.empty() &&
        (rc = ptmi_host_write_raw(c.error_map.c_str(), se_rgba.data(), c.width, c.height, err, sizeof(err)))) {
        std::fprintf(stderr, "%s\n", err);
        return 1;
    }
    if (!c.features.empty() &&
        (rc = ptmi_host_write_raw(c.features.c_str(), normals_rgba.data(), c.width, c.height, err, sizeof(err)))) {
        std::fprintf(stderr, "%s\n", err);
        return 1;
    }
    if (!c.sample_map.empty() &&
        (rc = ptmi_host_write_raw(c.sample_map.c_str(), counts_rgba.data(), c.width, c.height, err, sizeof(err)))) {
        std::fprintf(stderr, "%s\n", err);
        return 1;
    }
    if (c.have_target || !c.error_map.empty()) std::printf("samples_done %u relative_error %.6g\n", samples_done, rel_err);
    double traced = (double)n * samples_done;
    if (c.adaptive) {
        traced = 0.0;
        for (size_t i = 0; i < n; i++) traced += counts_rgba[4 * i];
        std::printf("adaptive mean_spp %.9g tiles_at_max %u\n", traced / (double)n, tiles_at_max);
    }
    const double build_s = std::chrono::duration<double>(t1 - t0).count();
    const double trace_s = std::chrono::duration<double>(t2 - t1).count();
    std::fprintf(stderr, "scene %s built in %.3f s; %dx%d x %d spp traced in %.3f s (%.1f Msamples/s); wrote %s\n",
                 scene.c_str(), build_s, c.width, c.height, (int)samples_done, trace_s,
                 traced / trace_s / 1e6, png.c_str());
    if (c.gpus > 1)
        std::fprintf(stderr,
                     "%d GPUs (%s split): prepare %.3f ms, render %.3f ms, combine %.3f ms, read-back %.3f ms\n",
                     c.gpus, c.split.c_str(), mt.prepare_ms, mt.render_ms, mt.combine_ms, mt.readback_ms);
    return 0;
}
