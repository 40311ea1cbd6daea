// ptmi_launch.h -- the host-side launch wrappers that the two kernel files define and ptmi_api.cpp calls,
// declared once for the API files, so the compiler checks each definition against its declaration.  The study
// ones exist in the study build only (PTMI_STUDY; a file that never names it reads 0 here and does not
// define them).
#pragma once
#include <hip/hip_runtime.h>

#include "ptmi_device.h"

namespace ptmi {
// ---- ptmi_kernels.hip: the path tracer ----
hipError_t launch_trace(const DevScene& S, int flags, uint32_t samples, const WorkPlan& WP, const double* seeds,
                        const double* sunf, double* sums, double* part, uint32_t* item_ctr, double* sq,
                        hipStream_t st);
hipError_t launch_reduce(const double* part, double* sums, const WorkPlan& WP, int W, int H, bool planes, double* sq,
                         hipStream_t st);
hipError_t launch_sunflower(double* out, uint32_t samples, hipStream_t st);
hipError_t launch_plane_normals(DevObject* objs, int n, hipStream_t st);
hipError_t launch_camera_terms(const DevScene& S, hipStream_t st);
hipError_t launch_hemi_table(double* out, int* mismatch, hipStream_t st);
hipError_t launch_features(const DevScene& S, double* feat, hipStream_t st);
hipError_t launch_features_chain(const DevScene& S, double* feat, uint32_t max_chain, double reflect_min,
                                 hipStream_t st);
const void* trace_kernel_symbol(int flags);
int trace_kernel_flags(int flags);
int trace_block_threads(int flags);
int trace_tiles_per_block(int flags);
#if PTMI_STUDY
hipError_t launch_tile_order(unsigned long long* cost, uint32_t n_whole, uint32_t n_tail, uint32_t stride,
                             uint32_t offset, uint32_t* order, hipStream_t st);
const void* trace_split_symbol(int flags);
const void* walk_split_symbol();
hipError_t launch_split_pass(const DevScene& S, int flags, uint32_t samples, const WorkPlan& WP, const SplitBufs& B,
                             const double* seeds, const double* sunf, double* part, uint32_t walk_grid,
                             hipStream_t st);
hipError_t launch_walk(const DevScene& S, int flags, int mode, const WalkReq* req, uint32_t n, WalkRes* res,
                       uint32_t* next, uint32_t grid, hipStream_t st);
const void* walk_kernel_symbol(int mode);
#endif
// the capture and timeline builds' hooks (hipErrorNotSupported in every other build)
hipError_t capture_setup(WalkReq* req, WalkRes* res, uint32_t cap);
hipError_t capture_count(uint32_t* n);
hipError_t timeline_setup(unsigned long long* buf, uint32_t cap);

// ---- ptmi_image_kernels.hip: the image-space passes ----
hipError_t launch_denoise(const double* rgba, const double* se, const double* feat, uint32_t W, uint32_t H,
                          uint32_t iterations, bool demod, double sigma_l, double sigma_d, uint32_t npow, double* out,
                          double* out_se, double* work, int variant, hipStream_t st);
hipError_t launch_reproject(const double* rgba, const double* se, const double* feat, const double* prev_hist,
                            const double* prev_feat, const ReprojectArgs& a, double* out_hist, double* out_rgba,
                            double* out_se, const double* motion, int32_t n_obj, hipStream_t st);
hipError_t launch_history_gather(const double* rgba, const double* se, const double* feat, const double* prev_hist,
                                 const double* prev_feat, const ReprojectArgs& a, double* gathered,
                                 const double* motion, int32_t n_obj, hipStream_t st);
hipError_t launch_rectify(const double* rgba, const double* se, const double* feat, const double* gathered,
                          const RectifyArgs& a, uint32_t radius, double* out_hist, double* out_rgba, double* out_se,
                          hipStream_t st);
hipError_t launch_variance(const double* rgba, const double* se, const double* feat, const double* prev_mom,
                           const double* prev_feat, const VarianceArgs& a, uint32_t radius, double* out_mom,
                           double* out_se, const double* motion, int32_t n_obj, hipStream_t st);
hipError_t launch_error_map(const double* sums, const double* sq, uint32_t W, uint32_t H, double* se, double* tile_err,
                            double* tile_part, double* stats, hipStream_t st);
hipError_t launch_accumulate(double* dst, const double* src, size_t n, hipStream_t st);
hipError_t launch_finalize(const double* sums, double* out, uint32_t npix, uint32_t samples, hipStream_t st);
hipError_t launch_finalize_counts(const double* sums, double* out, uint32_t npix, hipStream_t st);
hipError_t launch_select_tiles(const double* tile_err, const uint32_t* in_tiles, uint32_t n_in, double threshold,
                               uint32_t* out_tiles, uint32_t* count, hipStream_t st);
hipError_t launch_combine(const double* parts, uint32_t nparts, size_t npix, double* out, uint32_t samples,
                          hipStream_t st);
hipError_t launch_seeds(double* seeds, uint32_t n, uint64_t stream, hipStream_t st);
}  // namespace ptmi
