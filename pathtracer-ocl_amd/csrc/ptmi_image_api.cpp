// ptmi_image_api.cpp -- the image-space half of the C ABI (include/ptmi.h): the passes over frames in device
// memory that need no ptmi_scene.  Each entry point checks its arguments (ptmi_image_args.h for the passes with
// parameter records and buffer tables) and launches (ptmi_image_kernels.hip through ptmi_launch.h).  The passes
// that read a scene, ptmi_scene_features and ptmi_scene_features_chain, are in ptmi_api.cpp.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/ptmi_diag.h"
#include "ptmi_image_args.h"
#include "ptmi_launch.h"  // (PTMI_STUDY, never named here, reads 0 there)
#include "ptmi_motion.h"

using namespace ptmi;

// ptmi_diag_denoise_variant: the form of the a-trous pass (ptmi_image_kernels.hip launch_denoise).
static std::atomic<int> g_denoise_variant{1};  // the LDS form: 2.20 against 3.01 ms (profiles/denoise/SUMMARY.md)

extern "C" {

int ptmi_select_tiles(const double* tile_err_dev, const uint32_t* in_tiles_dev, uint32_t n_in, double threshold,
                      uint32_t* out_tiles_dev, uint32_t* count_dev, void* hip_stream, char* err, size_t err_len) {
    if (!count_dev || (n_in > 0 && (!tile_err_dev || !out_tiles_dev)) || n_in > (1u << 31) ||
        (n_in > 0 && out_tiles_dev == in_tiles_dev)) {
        set_err(err, err_len, "bad select-tiles arguments (%u candidates)", n_in);
        return PTMI_ERR_ARG;
    }
    HIP_TRY(launch_select_tiles(tile_err_dev, in_tiles_dev, n_in, threshold, out_tiles_dev, count_dev,
                                (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_finalize_counts(const double* sums_dev, double* out_dev, uint32_t n_pixels, void* hip_stream, char* err,
                         size_t err_len) {
    if (!sums_dev || !out_dev) {
        set_err(err, err_len, "bad finalize arguments");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(launch_finalize_counts(sums_dev, out_dev, n_pixels, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_finalize(const double* sums_dev, double* out_dev, uint32_t n_pixels, uint32_t samples, void* hip_stream,
                  char* err, size_t err_len) {
    if (!sums_dev || !out_dev || samples == 0) {
        set_err(err, err_len, "bad finalize arguments");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(launch_finalize(sums_dev, out_dev, n_pixels, samples, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_fill_seeds(double* seeds_dev, uint32_t n, uint64_t seed_stream, void* hip_stream, char* err,
                    size_t err_len) {
    if (!seeds_dev) {
        set_err(err, err_len, "seeds_dev == NULL");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(launch_seeds(seeds_dev, n, seed_stream, (hipStream_t)hip_stream));
    return PTMI_OK;
}

// The device-side combine of ptmi_trace_multi, for callers that gather their own partial
// frames (one per GPU) into one device buffer: slots summed in slot order, x 1/S, alpha 1.
int ptmi_combine_frames(const double* parts_dev, uint32_t n_parts, uint32_t n_pixels, double* out_dev,
                        uint32_t samples, void* hip_stream, char* err, size_t err_len) {
    if (!parts_dev || !out_dev || n_parts == 0 || samples == 0) {
        set_err(err, err_len, "bad combine arguments");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(launch_combine(parts_dev, n_parts, n_pixels, out_dev, samples, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_error_map(const double* sums_dev, const double* sq_dev, uint32_t width, uint32_t height, double* se_dev,
                   double* tile_err_dev, double* stats_dev, void* hip_stream, char* err, size_t err_len) {
    if (!sums_dev || !sq_dev || !stats_dev || width == 0 || height == 0) {
        set_err(err, err_len, "bad error-map arguments");
        return PTMI_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // The tiles' partial summaries between the two kernels: stream-ordered scratch.
    const size_t tiles = (size_t)((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile);
    double* tile_part = nullptr;
    HIP_TRY(hipMallocAsync((void**)&tile_part, tiles * 4 * sizeof(double), st));
    const hipError_t e = launch_error_map(sums_dev, sq_dev, width, height, se_dev, tile_err_dev, tile_part, stats_dev, st);
    HIP_TRY(hipFreeAsync(tile_part, st));
    HIP_TRY(e);
    return PTMI_OK;
}

int ptmi_accumulate(double* dst_dev, const double* src_dev, size_t n, void* hip_stream, char* err, size_t err_len) {
    if (!dst_dev || !src_dev) {
        set_err(err, err_len, "bad accumulate arguments");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(launch_accumulate(dst_dev, src_dev, n, (hipStream_t)hip_stream));
    return PTMI_OK;
}

size_t ptmi_denoise_work_bytes(uint32_t width, uint32_t height) { return denoise_work_bytes(width, height); }

int ptmi_denoise(const double* rgba_dev, const double* se_dev, const double* feat_dev, uint32_t width, uint32_t height,
                 const ptmi_denoise_params* params, double* out_rgba_dev, double* out_se_dev, void* work_dev,
                 size_t work_bytes, void* hip_stream, char* err, size_t err_len) {
    ptmi_denoise_params p;
    if (const int rc = check_denoise(rgba_dev, se_dev, feat_dev, width, height, params, out_rgba_dev, out_se_dev,
                                     work_dev, work_bytes, p, err, err_len))
        return rc;
    const bool demod = (p.flags & PTMI_DENOISE_DEMODULATE) != 0;  // (outside HIP_TRY: its message quotes the call)
    HIP_TRY(launch_denoise(rgba_dev, se_dev, feat_dev, width, height, p.iterations, demod, p.sigma_l, p.sigma_d, p.normal_power, out_rgba_dev,
                           out_se_dev, (double*)work_dev, g_denoise_variant.load(), (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_diag_denoise_variant(int variant) {
    if (variant < 0 || variant > 1) return -1;
    return g_denoise_variant.exchange(variant);
}

int ptmi_motion_table(const void* prev_objects, const void* cur_objects, uint32_t n_obj, double* motion_dev,
                      void* hip_stream, char* err, size_t err_len) {
    if (!prev_objects || !cur_objects || !motion_dev || n_obj == 0 || n_obj > PTMI_MAX_OBJECTS ||
        ((uintptr_t)motion_dev & 15u)) {
        set_err(err, err_len, "bad motion table arguments (%u objects; NULL or misaligned pointer)", n_obj);
        return PTMI_ERR_ARG;
    }
    double table[PTMI_MAX_OBJECTS * PTMI_MOTION_DOUBLES];
    for (uint32_t k = 0; k < n_obj; k++)
        motion_record((const uint8_t*)prev_objects + (size_t)PTMI_OBJECT_BYTES * k,
                      (const uint8_t*)cur_objects + (size_t)PTMI_OBJECT_BYTES * k, table + PTMI_MOTION_DOUBLES * k);
    // In stream order behind the work that still reads the buffer; `table` lives until the copy is done.
    const size_t bytes = (size_t)n_obj * PTMI_MOTION_DOUBLES * sizeof(double);  // (outside HIP_TRY: its message quotes the call)
    HIP_TRY(hipMemcpyAsync(motion_dev, table, bytes, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_reproject(const double* rgba_dev, const double* se_dev, const double* feat_dev, const double* prev_hist_dev,
                   const double* prev_feat_dev, const void* prev_camera, uint32_t width, uint32_t height,
                   const ptmi_reproject_params* params, double* out_hist_dev, double* out_rgba_dev, double* out_se_dev,
                   void* hip_stream, char* err, size_t err_len) {
    ReprojectArgs a;
    if (const int rc = check_reproject(rgba_dev, se_dev, feat_dev, prev_hist_dev, prev_feat_dev, prev_camera, width,
                                       height, params, out_hist_dev, out_rgba_dev, out_se_dev, nullptr, 0, a, err, err_len))
        return rc;
    HIP_TRY(launch_reproject(rgba_dev, se_dev, feat_dev, prev_hist_dev, prev_feat_dev, a, out_hist_dev, out_rgba_dev,
                             out_se_dev, nullptr, 0, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_reproject_motion(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                          const double* prev_hist_dev, const double* prev_feat_dev, const void* prev_camera,
                          uint32_t width, uint32_t height, const ptmi_reproject_params* params, double* out_hist_dev,
                          double* out_rgba_dev, double* out_se_dev, const double* motion_dev, uint32_t n_obj,
                          void* hip_stream, char* err, size_t err_len) {
    if (!motion_dev || n_obj == 0 || n_obj > PTMI_MAX_OBJECTS) {
        set_err(err, err_len, "bad reproject arguments (motion table NULL or of %u objects)", n_obj);
        return PTMI_ERR_ARG;
    }
    ReprojectArgs a;
    if (const int rc = check_reproject(rgba_dev, se_dev, feat_dev, prev_hist_dev, prev_feat_dev, prev_camera, width, height,
                                       params, out_hist_dev, out_rgba_dev, out_se_dev, motion_dev, n_obj, a, err, err_len))
        return rc;
    HIP_TRY(launch_reproject(rgba_dev, se_dev, feat_dev, prev_hist_dev, prev_feat_dev, a, out_hist_dev, out_rgba_dev,
                             out_se_dev, motion_dev, (int32_t)n_obj, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_history_gather(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                        const double* prev_hist_dev, const double* prev_feat_dev, const void* prev_camera,
                        uint32_t width, uint32_t height, const ptmi_reproject_params* params, double* gathered_dev,
                        const double* motion_dev, uint32_t n_obj, void* hip_stream, char* err, size_t err_len) {
    if (const int rc = check_optional_motion("history_gather", motion_dev, n_obj, err, err_len)) return rc;
    ReprojectArgs a;
    if (const int rc = check_reproject(rgba_dev, se_dev, feat_dev, prev_hist_dev, prev_feat_dev, prev_camera, width, height,
                                       params, gathered_dev, nullptr, nullptr, motion_dev, n_obj, a, err, err_len))
        return rc;
    HIP_TRY(launch_history_gather(rgba_dev, se_dev, feat_dev, prev_hist_dev, prev_feat_dev, a, gathered_dev, motion_dev,
                                  (int32_t)n_obj, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_rectify(const double* rgba_dev, const double* se_dev, const double* feat_dev, const double* gathered_dev,
                 uint32_t width, uint32_t height, const ptmi_rectify_params* params, double* out_hist_dev,
                 double* out_rgba_dev, double* out_se_dev, void* hip_stream, char* err, size_t err_len) {
    RectifyArgs a;
    uint32_t radius;
    if (const int rc = check_rectify(rgba_dev, se_dev, feat_dev, gathered_dev, width, height, params, out_hist_dev,
                                     out_rgba_dev, out_se_dev, a, radius, err, err_len))
        return rc;
    HIP_TRY(launch_rectify(rgba_dev, se_dev, feat_dev, gathered_dev, a, radius, out_hist_dev, out_rgba_dev, out_se_dev,
                           (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_variance_estimate(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                           const double* prev_mom_dev, const double* prev_feat_dev, const void* prev_camera,
                           uint32_t width, uint32_t height, const ptmi_variance_params* params, double* out_mom_dev,
                           double* out_se_dev, const double* motion_dev, uint32_t n_obj, void* hip_stream, char* err,
                           size_t err_len) {
    VarianceArgs a;
    uint32_t radius;
    if (const int rc = check_variance(rgba_dev, se_dev, feat_dev, prev_mom_dev, prev_feat_dev, prev_camera, width, height,
                                      params, out_mom_dev, out_se_dev, motion_dev, n_obj, a, radius, err, err_len))
        return rc;
    HIP_TRY(launch_variance(rgba_dev, se_dev, feat_dev, prev_mom_dev, prev_feat_dev, a, radius, out_mom_dev, out_se_dev,
                            motion_dev, (int32_t)n_obj, (hipStream_t)hip_stream));
    return PTMI_OK;
}

}  // extern "C"
