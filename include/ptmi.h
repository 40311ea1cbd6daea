/*
 * ptmi.h -- C ABI of libptmi.so, the MI355X (gfx950) path-tracing backend that
 * replaces the reference's OpenCL host driver + kernel
 * (eriklupander/pathtracer-ocl  internal/ocl/ocltracer.go + internal/ocl/tracer.cl).
 *
 * The input records are consumed BYTE-FOR-BYTE in the reference's packed layouts:
 *   objects   : n_obj * 1024 B  CLObject   (ocltracer.go:25-51  == tracer.cl:37-63)
 *   triangles : n_tri *  512 B  CLTriangle (ocltracer.go:66-78  == tracer.cl:82-93)
 *   groups    : n_grp *  256 B  CLGroup    (ocltracer.go:53-64  == tracer.cl:24-35)
 *   camera    :          256 B  CLCamera   (ocltracer.go:85-96  == tracer.cl:6-17)
 * so a cgo caller passes &slice[0] of the slices BuildSceneBufferCL returns
 * (see INTEGRATION.md).  No pointer is retained after a call returns.
 *
 * Output: float64 RGBA, row-major, W*H*4 values, RGB = sum of samples / samples,
 * A = 1.0 (tracer.cl:1184-1187).
 *
 * Every entry point returns PTMI_OK (0) or a negative PTMI_ERR_* code and, when
 * `err` is non-NULL, a NUL-terminated message.  There is no silent fallback:
 * without a usable gfx950 device the calls fail.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_ABI_VERSION 1
#define PTMI_OBJECT_BYTES 1024
#define PTMI_TRIANGLE_BYTES 512
#define PTMI_GROUP_BYTES 256
#define PTMI_CAMERA_BYTES 256
#define PTMI_MAX_OBJECTS 16 /* tracer.cl:846 `__local object objects[16]` */

enum {
    PTMI_OK = 0,
    PTMI_ERR_ARG = -1,         /* bad sizes / NULL pointers / out-of-range indices   */
    PTMI_ERR_DEVICE = -2,      /* no such device, or not a gfx950 device            */
    PTMI_ERR_HIP = -3,         /* a HIP runtime call failed                          */
    PTMI_ERR_UNSUPPORTED = -4, /* input outside what this build implements (e.g. BVH too deep) */
    PTMI_ERR_NOMEM = -5
};

/* Texture arrays of ocl.Trace (textures / sphereTextures / cubeTextures,
 * ocltracer.go:178-183, 228-254): array k holds count[k] layers of
 * width[k] x height[k] NRGBA8 pixels (image.NRGBA.Pix, rows top to bottom), the
 * layers concatenated in slice order -- exactly the bytes prepareTextures hands
 * to clCreateImage.  [0] backs plane colours and plane normal maps, [1] sphere
 * colours (sphericalMap), [2] cube colours (cubeUV cross), tracer.cl:907-914,
 * 1077-1092.  A NULL struct or count 0 is the reference's all-zero fake image.
 * Sampling follows the kernel's sampler (tracer.cl:829): normalized
 * coordinates, CLK_ADDRESS_REPEAT, CLK_FILTER_LINEAR, UNORM8 -> c/255, layer =
 * clamp(rint(index), 0, count-1) -- in software (OpenCL 1.2 s8.2 formulas, FP32):
 * gfx950 has no image instructions (DESIGN.md "Textures").  Pixels are copied to the
 * device during the call; the pointers are not retained. */
typedef struct ptmi_textures {
    const uint8_t* pixels[3];
    uint32_t width[3], height[3], count[3];
} ptmi_textures;

/*
 * ptmi_trace -- drop-in for `func Trace(objects []CLObject, triangles []CLTriangle,
 *   groups []CLGroup, deviceIndex, samples int, camera CLCamera, textures,
 *   sphereTextures, cubeTextures []image.Image) []float64`   (ocltracer.go:100-226).
 *
 *  - empty triangle / group slices are allowed (n = 0): the reference pads them
 *    with one zero record (ocltracer.go:106-120), which is equivalent;
 *  - device_index < 0 selects device 0 (ocltracer.go:138-140), an index past the
 *    last device is an error (ocltracer.go:135-137: logrus.Fatalf);
 *  - seeds: W*H per-pixel seeds in [0,1), row-major (the reference draws one
 *    rand.Float64() per pixel, ocltracer.go:260-263).  NULL -> generated from
 *    `seed_stream` (Go-Float64 granularity k/2^53, SplitMix64-derived);
 *  - the frame is rendered in one resident launch sequence (the reference's 4-row
 *    batches exist only to dodge a display watchdog, ocltracer.go:212-213).
 */
int ptmi_trace(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
               const void* groups, uint32_t n_grp, int device_index, uint32_t samples,
               const void* camera, const double* seeds, uint64_t seed_stream,
               const ptmi_textures* textures, double* out_rgba, char* err, size_t err_len);

/*
 * ptmi_trace_multi -- ptmi_trace over several GPUs of this process:
 * one host thread per entry of devices[0..n_devices) (an index may repeat), each
 * rendering its shard of the frame into its own partial sums:
 *   split 0 (sample): device d renders a contiguous range of sample indices of
 *                     every pixel (global indices, as ptmi_scene_render), balanced
 *                     by cost: late indices weigh ~4 % more (ptmi/dist.py);
 *   split 1 (tile)  : device d renders every sample of the 8x8 tiles t with
 *                     t % n == d.
 * The host converts the scene and builds its traversal index once; each device
 * uploads it.  The partial frames are combined on the device side: peer copies
 * over xGMI into a gather buffer on devices[0], summed there in device order
 * (deterministic) and normalised as ptmi_finalize, then read back once.  The
 * result equals ptmi_trace's up to FP64 summation order: each device plans its own
 * work items (ptmi_scene_render, chunks = 0), and where that plan splits a tile's
 * samples into chunks differently from the one-device plan, the tile's per-pixel
 * sums are added in a different grouping (bit-identical when every tile is one
 * whole item on both sides, e.g. short sample ranges).  Same record / seed / error contract as ptmi_trace.  (The
 * torch.distributed driver, bench.py, does the same with one process per GPU and
 * an RCCL reduce.)
 */
int ptmi_trace_multi(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                     const void* groups, uint32_t n_grp, const int* devices, uint32_t n_devices, int split,
                     uint32_t samples, const void* camera, const double* seeds, uint64_t seed_stream,
                     const ptmi_textures* textures, double* out_rgba, char* err, size_t err_len);

/* Wall-clock phases of one ptmi_trace_multi call (milliseconds). */
typedef struct ptmi_multi_timing {
    double prepare_ms;  /* host: record conversion + traversal-index build, once for all devices */
    double render_ms;   /* until the slowest device has its partial frame: upload, seeds, kernels */
    double combine_ms;  /* from then: xGMI peer copies into the first device + the ordered sum */
    double readback_ms; /* the RGBA frame to host memory */
    double total_ms;    /* the whole call, releasing the device buffers included */
    int32_t peer_direct; /* shards on other devices with direct peer (xGMI) access to devices[0] */
    int32_t peer_staged; /* shards on other devices whose copy the runtime stages (peer access refused) */
} ptmi_multi_timing;

/* ptmi_trace_multi, also reporting its phases in *timing (may be NULL). */
int ptmi_trace_multi_timed(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                           const void* groups, uint32_t n_grp, const int* devices, uint32_t n_devices, int split,
                           uint32_t samples, const void* camera, const double* seeds, uint64_t seed_stream,
                           const ptmi_textures* textures, double* out_rgba, ptmi_multi_timing* timing, char* err,
                           size_t err_len);

/* The combine step of ptmi_trace_multi, for callers that gather their own partial
 * frames: parts_dev holds n_parts frames of n_pixels * 4 doubles (RGB sums, A = the
 * sample count) back to back on one device; out_dev[4i + c] = (sum over parts, in part
 * order, of part[4i + c]) * (1.0 / samples) for RGB and 1.0 for A (tracer.cl:1184-1187).
 * out_dev may alias parts_dev (slot 0).  Asynchronous on hip_stream. */
int ptmi_combine_frames(const double* parts_dev, uint32_t n_parts, uint32_t n_pixels, double* out_dev,
                        uint32_t samples, void* hip_stream, char* err, size_t err_len);

/* First sample index of device g of n in ptmi_trace_multi's cost-balanced sample
 * split (g = n -> samples); the same table as bench.py's ranks (ptmi/dist.py). */
uint32_t ptmi_sample_split_point(int g, int n, uint32_t samples);

/* --list-devices (cmd/pt/main.go:98-112). */
int ptmi_device_count(void);
int ptmi_device_name(int device_index, char* buf, size_t len);

/* ------------------------------------------------------------------------
 * Resident-scene API: the scene is converted and uploaded to HBM once, frames
 * are rendered from device-resident seeds into device-resident sums on a
 * caller-supplied HIP stream (hipStream_t passed as void*).  Used by bench.py,
 * the multi-GPU driver and any caller that renders several frames / sample
 * ranges per scene.  All device pointers are allocations on the scene's device.
 * ------------------------------------------------------------------------ */
typedef struct ptmi_scene ptmi_scene;

int ptmi_scene_create(int device_index, const void* objects, uint32_t n_obj, const void* triangles,
                      uint32_t n_tri, const void* groups, uint32_t n_grp, const void* camera,
                      ptmi_scene** out, char* err, size_t err_len);
/* ptmi_scene_create with the scene's texture arrays (see ptmi_textures; NULL =
 * no textures).  ptmi_scene_create(...) == ptmi_scene_create_textured(..., NULL, ...). */
int ptmi_scene_create_textured(int device_index, const void* objects, uint32_t n_obj, const void* triangles,
                               uint32_t n_tri, const void* groups, uint32_t n_grp, const void* camera,
                               const ptmi_textures* textures, ptmi_scene** out, char* err, size_t err_len);
void ptmi_scene_destroy(ptmi_scene* s);
int ptmi_scene_size(const ptmi_scene* s, uint32_t* width, uint32_t* height);

/*
 * Render samples [sample_begin, sample_end) of a `samples`-spp frame.
 *   seeds_dev  : W*H doubles
 *   sums_dev   : W*H*4 doubles, OVERWRITTEN with RGB sums over the sample range
 *                (A = number of samples) for owned pixels, 0 for the others.
 *   tile_stride/tile_offset: pixel ownership for a tile split -- 8x8 tile t is
 *                owned when t % tile_stride == tile_offset (1/0 = all pixels).
 *   chunks     : sample chunks per pixel for every owned tile (load balance), or
 *                0 = auto: most tiles are one work item over the whole range
 *                (summed in sample order), the tiles at the end of the launch are
 *                split into chunks; mesh scenes chunk every tile.  Chunk sums are
 *                combined in a fixed order, so results are deterministic.  The
 *                affine mesh kernels hand a work item's (pixel, sample) paths to
 *                whichever lanes are free (the path pool) and add a pixel's paths
 *                in completion order: every path is the reference's, the sums
 *                differ from sample order only by FP64 rounding, and a render
 *                is reproducible bit for bit.
 * Sample indices are GLOBAL (fgi2 = seed/samples and the DoF aperture pattern
 * depend on n and on the total, tracer.cl:841, 766), so any split of
 * [0, samples) sums to the same frame.
 */
int ptmi_scene_render(ptmi_scene* s, uint32_t samples, uint32_t sample_begin, uint32_t sample_end,
                      uint32_t tile_stride, uint32_t tile_offset, const double* seeds_dev,
                      double* sums_dev, uint32_t chunks, void* hip_stream, char* err, size_t err_len);

/*
 * ptmi_scene_render, also writing sq_dev[W*H]: for owned pixels the sum over the
 * range's paths of (r*r + g*g) + b*b of the path's colour (separately rounded
 * FP64, added where and in the order the colour is added), 0 for the others.
 * sums_dev is bit-identical to ptmi_scene_render's for the same arguments: the
 * work plan, chunks and tile ownership are the same.  A NaN path colour makes
 * the pixel's entry NaN, as it makes its sums NaN.  Timing and the RNG mode
 * apply as to ptmi_scene_render.  PTMI_ERR_ARG when a work item of a pooled
 * (affine mesh, parity mode) scene would hold 2^26 samples or more: pass more
 * chunks.
 */
int ptmi_scene_render_moments(ptmi_scene* s, uint32_t samples, uint32_t sample_begin, uint32_t sample_end,
                              uint32_t tile_stride, uint32_t tile_offset, const double* seeds_dev,
                              double* sums_dev, double* sq_dev, uint32_t chunks, void* hip_stream,
                              char* err, size_t err_len);

/*
 * ptmi_scene_render_moments on a caller's list of 8x8 tiles (per-tile adaptive sampling):
 * tiles_dev holds n_tiles distinct raster indices of tiles, in device memory.  sums_dev
 * (W*H*4) and sq_dev (W*H, required) are OVERWRITTEN: the listed tiles' pixels get what
 * ptmi_scene_render_moments(..., tile_stride 1, tile_offset 0, the same chunks) gives them
 * (bit for bit with an explicit chunk count; with chunks = 0 the plan depends on the
 * number of tiles, so the sums may differ by FP64 regrouping), every other pixel 0.  An
 * index >= the frame's tile count is skipped; duplicate entries are undefined behaviour.
 * n_tiles == 0 zeroes both buffers and launches no trace kernel; tiles_dev == NULL with
 * n_tiles > 0 is PTMI_ERR_ARG.  The work items run in list order (the costliest-first
 * dispatch order of mesh scenes is built for the library's own tile ownership only).
 * Asynchronous on the stream; timing, the RNG mode and the 2^26 pooled-item guard apply
 * as to ptmi_scene_render_moments.
 */
int ptmi_scene_render_tiles(ptmi_scene* s, uint32_t samples, uint32_t sample_begin, uint32_t sample_end,
                            const uint32_t* tiles_dev, uint32_t n_tiles, const double* seeds_dev,
                            double* sums_dev, double* sq_dev, uint32_t chunks, void* hip_stream, char* err,
                            size_t err_len);

/*
 * The tiles that still need samples: an order-preserving compaction of the candidates
 * in_tiles_dev[0..n_in) (in_tiles_dev == NULL: tiles 0..n_in themselves; n_in <= 2^31).
 * Candidate t is kept iff tile_err_dev[t] > threshold: a NaN error is dropped (it would
 * never converge), +inf is kept, an error equal to the threshold is dropped.  Every
 * candidate must index tile_err_dev.  The kept tiles go to out_tiles_dev (room for n_in
 * entries) in candidate order, their number to count_dev[0]; n_in == 0 writes count 0.
 * out_tiles_dev must not alias in_tiles_dev (callers ping-pong two buffers).  One
 * workgroup, no atomics: equal inputs give equal lists.  Asynchronous on the stream.
 */
int ptmi_select_tiles(const double* tile_err_dev, const uint32_t* in_tiles_dev, uint32_t n_in,
                      double threshold, uint32_t* out_tiles_dev, uint32_t* count_dev, void* hip_stream,
                      char* err, size_t err_len);

/*
 * ptmi_finalize by each pixel's own sample count n = sums_dev[4i+3] (frames whose tiles
 * stopped at different counts): n == 0 -> RGB 0, otherwise RGB = sum_c * (1.0 / n), the
 * same multiply as ptmi_finalize, so a uniform count gives its output bit for bit; A = 1.0.
 * out_dev must not alias sums_dev.
 */
int ptmi_finalize_counts(const double* sums_dev, double* out_dev, uint32_t n_pixels, void* hip_stream,
                         char* err, size_t err_len);

/*
 * The standard error of each pixel's mean from frame sums (r, g, b, n per pixel)
 * and second moments.  Per pixel i, n = sums_dev[4i+3]:
 *   n == 0: se = 0 (not owned);  n == 1: se = +inf;  otherwise
 *   mean_c = sum_c / n
 *   d   = sq[i] / n - ((mean_r*mean_r + mean_g*mean_g) + mean_b*mean_b)
 *   var = max(d, 0) * (n / (n - 1)),   se = sqrt(var / n)
 * (the root of the three channels' summed variances of the mean).
 *   se_dev[W*H]        se per pixel (may be NULL)
 *   tile_err_dev[t]    per 8x8 tile, raster order: sqrt(mean of se^2 over the
 *                      tile's in-image pixels with n >= 2), 0 when none (may be NULL)
 *   stats_dev[0..4)    over all pixels with n >= 2: sqrt(mean se^2); the largest
 *                      finite se; the mean of (mean_r + mean_g + mean_b) / 3;
 *                      their number
 * Both reductions run in a fixed order: equal inputs give equal bits.
 */
int ptmi_error_map(const double* sums_dev, const double* sq_dev, uint32_t width, uint32_t height,
                   double* se_dev, double* tile_err_dev, double* stats_dev, void* hip_stream,
                   char* err, size_t err_len);

/*
 * First-hit feature buffers (an AOV pass): what the camera ray through each pixel's centre hits.
 * feat_dev gets W*H*PTMI_FEATURE_DOUBLES doubles, row-major, one record per pixel:
 *   [0..2] world position of the closest hit     [3] its t along the normalised ray direction
 *   [4..6] world shading normal, unit, facing the eye (plane normal maps and interpolated
 *          triangle normals included)            [7] the object's index in the caller's list
 *                                                    as a double, -1.0 on a miss
 *   [8..10] albedo: the object, triangle or texture colour the path's mask would be multiplied by
 *          (an emissive object's colour too)     [11] 0.0
 * The ray is the pinhole one (the aperture is ignored, so depth of field is not in these buffers),
 * and the hit is the one the trace kernels pick for that ray, ties included.  Nothing here depends
 * on seeds, sample counts or the RNG mode.  A miss writes id -1 and zeros elsewhere.  feat_dev must
 * be 16-byte aligned.  Asynchronous on the stream.
 */
#define PTMI_FEATURE_DOUBLES 12
int ptmi_scene_features(ptmi_scene* s, double* feat_dev, void* hip_stream, char* err, size_t err_len);

/*
 * Specular-chain feature buffers: the same records, for the first surface behind mirrors and glass.
 * The pinhole ray is followed deterministically from its first hit to the first surface that is not
 * specular, and that surface is recorded at its virtual position, unfolded along the camera ray, so
 * the image in a planar mirror has the records of the mirrored scene.  Per pixel, with inside = false,
 * L = 0, tint m = (1, 1, 1), U = I (3x3) and k = 0, at each hit (t, pos, eye-facing unit normal n and
 * colour c as above, textures included) L += t, then the first rule that applies:
 *   1. final, if the object is emissive (emission[0] > 0) or k == max_chain;
 *   2. reflect, if reflectivity >= reflect_min: rd = rd - 2 (rd . n) n from pos,
 *      m *= c (the bounce record of a reflection tints the path), U = U (I - 2 n n^T), k++;
 *   3. thin glass (refractive index -1): straight on from pos, k++;
 *   4. glass (refractive index != 1): with s2 = nr^2 (1 - (n . eye)^2), nr = ri when inside and 1 / ri
 *      otherwise, total internal reflection (s2 > 1) takes rule 2's step; otherwise the refracted
 *      direction from pos, inside flips, k++ (no tint);
 *   5. final otherwise.
 * A segment starts at pos itself (the trace kernels start EPSILON off the surface along n): no hit is
 * taken at t <= EPSILON, so the surface just left is not met again, and the unfolded ray is the true one.
 * The final record: [0..2] = origin + rd0 * L, [3] = L, [4..6] = U n negated where it does not
 * face -rd0, [7] the final object's index, [8..10] = m * c, [11] = k as a double.  A miss on any
 * segment, or a direction that is not finite, writes id -1, zeros in [0..10] and k in [11].  A pixel
 * with k == 0 has ptmi_scene_features' record bit for bit.  The virtual position is exact for chains
 * of planar mirrors and approximate for curved mirrors and refraction; a pixel follows one branch
 * (glass is guided by what is behind it, not by its Fresnel reflection).
 * PTMI_ERR_ARG (and no launch) for a NULL scene or buffer, a buffer that is not 16-byte aligned,
 * max_chain outside [1, 16], or reflect_min NaN or outside (0, 1].  Allocates nothing; asynchronous
 * on the stream.
 */
int ptmi_scene_features_chain(ptmi_scene* s, double* feat_dev, uint32_t max_chain, double reflect_min,
                              void* hip_stream, char* err, size_t err_len);

/*
 * A variance-guided, edge-avoiding a-trous wavelet filter (the spatial part of SVGF) over a frame:
 *   rgba_dev  the frame (ptmi_finalize / ptmi_finalize_counts), W*H*4
 *   se_dev    its standard-error map (ptmi_error_map), W*H: the filter's variance is se^2
 *   feat_dev  the first-hit records (ptmi_scene_features)
 * `iterations` passes with 5x5 B3-spline taps at distance 2^i; a tap's weight falls with the angle
 * between the normals (cos^(2^normal_power)), with the tap's distance from the centre's tangent
 * plane (sigma_d, relative to the hit's t) and with the luminance difference against the local
 * standard deviation (sigma_l); hits and misses never mix.  With PTMI_DENOISE_DEMODULATE the colour
 * is divided by max(albedo, 1e-3) before the passes and multiplied back after them, so texture detail
 * is not blurred.  A pixel whose colour or se is not finite is copied through and read by no
 * neighbour.  out_rgba_dev (W*H*4, A = 1.0) must not alias rgba_dev; out_se_dev (W*H, may be NULL)
 * gets the filtered standard error.  The exact operation order is ptmi/denoise.py atrous_reference.
 * work_dev: ptmi_denoise_work_bytes(W, H) bytes of scratch on the same device (two ping-pong
 * states); work_dev, rgba_dev, feat_dev and out_rgba_dev must be 16-byte aligned.  Allocates
 * nothing; asynchronous on the stream.  PTMI_ERR_ARG (and no launch) for NULL pointers, iterations
 * outside 1..8, normal_power above 16, unknown flags, negative or non-finite sigmas, a short
 * workspace or aliased frames.
 */
#define PTMI_DENOISE_DEMODULATE 1u
typedef struct ptmi_denoise_params {
    uint32_t iterations;   /* a-trous passes, step 2^i; default 5, 1..8 */
    uint32_t flags;        /* PTMI_DENOISE_DEMODULATE = 1 (default on) */
    double sigma_l;        /* luminance: default 4.0  */
    double sigma_d;        /* plane distance, relative to the hit's t: default 0.01 */
    uint32_t normal_power; /* w_n = max(0, n_p.n_q)^(2^k), k = normal_power: default 7 (exponent 128) */
    uint32_t reserved;
} ptmi_denoise_params;

size_t ptmi_denoise_work_bytes(uint32_t width, uint32_t height);
int ptmi_denoise(const double* rgba_dev, const double* se_dev, const double* feat_dev, uint32_t width,
                 uint32_t height, const ptmi_denoise_params* params /* NULL = defaults */, double* out_rgba_dev,
                 double* out_se_dev /* may be NULL */, void* work_dev, size_t work_bytes, void* hip_stream,
                 char* err, size_t err_len);

/*
 * Temporal accumulation (the temporal part of SVGF): this frame blended into the history of the
 * surface points it shows, found in the previous frame by reprojecting each pixel's first hit.
 *   rgba_dev, se_dev, feat_dev   this frame, its standard-error map and its first-hit records
 *                                (ptmi_finalize, ptmi_error_map, ptmi_scene_features)
 *   prev_hist_dev, prev_feat_dev the previous frame's history (an earlier call's out_hist_dev) and
 *                                records; prev_hist_dev == NULL: the first frame, every pixel resets
 *                                (prev_feat_dev and prev_camera may then be NULL too)
 *   prev_camera                  HOST pointer to the previous frame's 256-byte CLCamera; its `inverse`
 *                                is inverted on the host (FP64 cofactors) into the world-to-camera matrix
 *   out_hist_dev                 W*H*PTMI_HISTORY_DOUBLES doubles per pixel: [0..2] the accumulated colour,
 *                                [3] its variance (se^2), [4] the history length N, [5..7] 0
 *   out_rgba_dev (may be NULL)   (accumulated colour, 1.0): with out_se_dev what ptmi_denoise takes
 *   out_se_dev   (may be NULL)   sqrt(variance)
 * A pixel RESETS to (rgb, se^2, N = 1) when there is no history, when it is a miss, when its point lies
 * behind the previous camera or its accepted bilinear weight W is below min_weight (or 0); a pixel whose
 * colour or se is not finite resets with N = 0 and is read by no later frame.  Otherwise, over the four
 * bilinear taps around the point's place in the previous image that are inside it, hold history
 * (N > 0, finite), show the same object, and pass the normal and plane-distance tests below:
 *   W = sum w;  h_c = rgb + (sum w (c_q - rgb)) / W;  h_var = (sum w^2 var_q) / W^2;  h_N = (sum w N_q) / W;
 *   N' = min(h_N + 1, max_history),  a = 1 / N';  colour' = h_c + a (rgb - h_c);
 *   var' = a^2 se^2 + (1 - a)^2 h_var.
 * h_c is the taps' weighted mean sum w c_q / W, computed around this frame's colour: in that order a
 * sequence of equal colours stays equal bit for bit whatever the rounding of the projected place, which
 * the plain quotient does not give.  The exact operation order is ptmi/temporal.py reproject_reference.  The variance formula takes the
 * frames for INDEPENDENT estimates: render them with different seeds.  Two frames with equal seeds and
 * an unchanged camera are the same estimate, and averaging them halves nothing.
 * The guides are the pinhole ray through the pixel centre: the first hit on glass or a mirror
 * reprojects the glass, not what shows through it, and the history is trusted wherever the geometry
 * matches: view-dependent shading and changed lighting are the business of ptmi_history_gather +
 * ptmi_rectify, which test the history against the frame; the objects are taken to stand still, only the
 * camera moves (ptmi_reproject_motion follows objects that moved); at 1 spp the rendered se is +inf
 * and every pixel resets: pass ptmi_variance_estimate's map instead.
 * Allocates nothing; asynchronous on the stream.  No output may overlap an input or another output, in
 * whole or in part (callers ping-pong two history buffers; there is no in-place form: out_rgba_dev is
 * not rgba_dev, out_se_dev is not se_dev); the ranges are checked.  Every buffer but se_dev and
 * out_se_dev must be 16-byte aligned.
 * PTMI_ERR_ARG (no launch, no device call) for a NULL required pointer, zero width or height,
 * max_history outside 1..65536, non-zero flags, a negative or non-finite threshold, overlapping or
 * misaligned buffers, and a prev_camera that is singular, not finite or of another width or height.
 */
#define PTMI_HISTORY_DOUBLES 8
typedef struct ptmi_reproject_params {
    uint32_t max_history; /* default 32; 1..65536 */
    uint32_t flags;       /* 0 */
    double normal_cos;    /* default 0.9 : a tap is rejected when n_p . n_q <  normal_cos */
    double plane_dist;    /* default 0.02: ... when |n_p . (x_q - x_p)| > plane_dist * t_p */
    double min_weight;    /* default 0.05: history is dropped when the accepted bilinear weight is below it */
} ptmi_reproject_params;

int ptmi_reproject(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                   const double* prev_hist_dev, const double* prev_feat_dev, const void* prev_camera,
                   uint32_t width, uint32_t height, const ptmi_reproject_params* params /* NULL = defaults */,
                   double* out_hist_dev, double* out_rgba_dev /* may be NULL */, double* out_se_dev /* may be NULL */,
                   void* hip_stream, char* err, size_t err_len);

/* dst_dev[k] += src_dev[k] over n doubles, on the caller's stream: batches of sums
 * (A included, so the sample counts add) and of second moments. */
int ptmi_accumulate(double* dst_dev, const double* src_dev, size_t n, void* hip_stream, char* err,
                    size_t err_len);

/* out_dev[i] = sums_dev[i] * (1.0 / samples) for RGB, 1.0 for A (tracer.cl:837,1184-1187). */
int ptmi_finalize(const double* sums_dev, double* out_dev, uint32_t n_pixels, uint32_t samples,
                  void* hip_stream, char* err, size_t err_len);

/* Fill seeds_dev[0..n) with the generator ptmi_trace uses for seeds == NULL. */
int ptmi_fill_seeds(double* seeds_dev, uint32_t n, uint64_t seed_stream, void* hip_stream, char* err,
                    size_t err_len);

/* Random numbers of the scene's renders.  PTMI_RNG_NOISE3D (the default) is the
 * reference's noise3D hash (tracer.cl:314-317, called at :869, 982, 993, 1014, 1038,
 * 1057), bit for bit: images equal the reference kernel's.  PTMI_RNG_XOSHIRO is an
 * opt-in STATISTICAL mode: the same uniforms drawn from xoshiro128**, one stream per
 * (pixel, sample) path seeded from the pixel's seed and the sample index (32-bit hash),
 * so images are deterministic and independent of the work split, and converge to the
 * same expectation as the parity mode, but do not equal the reference's.  Affine,
 * untextured scenes only (else PTMI_ERR_UNSUPPORTED). */
enum { PTMI_RNG_NOISE3D = 0, PTMI_RNG_XOSHIRO = 1 };
int ptmi_scene_set_rng(ptmi_scene* s, int mode, char* err, size_t err_len);

/* A new camera (256-byte CLCamera) on a resident scene.  Afterwards the scene is what
 * ptmi_scene_create gives for the same objects, triangles, groups and textures with this camera:
 * every later render, moment render, tile render and feature pass is bit-identical to the fresh
 * scene's.  Nothing but the camera is converted or uploaded: the record, its origin (the create
 * call's own arithmetic), the kernel instantiation it selects (depth of field, affine or not -- a
 * camera can move a scene between instantiations), the camera terms behind the record, and, for mesh
 * scenes, the tile classes and the dispatch order.  Width and height must be the scene's (buffers and
 * work plans depend on them): else, or for a NULL scene or record, PTMI_ERR_ARG.  In the statistical
 * RNG mode a camera that makes the scene non-affine is PTMI_ERR_UNSUPPORTED.  Everything is checked
 * before anything changes: after PTMI_ERR_ARG or PTMI_ERR_UNSUPPORTED the scene renders exactly as
 * before.  PTMI_ERR_HIP (a runtime call failed during the update) may leave the record, the flags and
 * the tile classes partly updated: set the camera again, or destroy the scene.
 * HOST-BLOCKING: the call waits for all earlier work of the device (renders in flight read the camera
 * record in device memory) and returns after the upload and the terms pass have completed. */
int ptmi_scene_set_camera(ptmi_scene* s, const void* camera, char* err, size_t err_len);

/* New object records (n_obj * 1024-byte CLObject) on a resident scene: objects move, turn, change colour
 * or material between frames without a new traversal index.  Afterwards the scene is what
 * ptmi_scene_create gives for these objects with the scene's own triangles, groups, camera and textures:
 * every later render, moment render, tile render and feature pass is bit-identical to the fresh scene's.
 * May change: transform, inverse and inverse_transpose (taken from the record as given, as at creation),
 * colour, emission, reflectivity, refractive index, min_y / max_y and the texture fields.  Must NOT
 * change: n_obj, each object's type, and for a group object childCount, its child roots and bb_min /
 * bb_max (the traversal index of a mesh is built from them, in the group's own space; the transform is
 * not part of it): PTMI_ERR_ARG.  Re-derived, by the code the create call runs: the device objects and
 * their plane normals, the compact plane and sphere records, the kernel instantiation (materials, affine
 * or not, textured -- objects can move a scene between instantiations), the camera terms and the tiles'
 * candidate masks, and for mesh scenes the tile classes and the dispatch order.  In the statistical RNG
 * mode objects that make the scene non-affine or textured are PTMI_ERR_UNSUPPORTED.  Everything is
 * checked before anything changes: after PTMI_ERR_ARG or PTMI_ERR_UNSUPPORTED the scene renders exactly
 * as before.  PTMI_ERR_HIP (a runtime call failed during the update) may leave the records, the flags
 * and the terms partly updated: set the objects again, or destroy the scene.  (A flag set forced with
 * ptmi_diag_force_flags stays the one the scene was created under.)
 * HOST-BLOCKING, as ptmi_scene_set_camera: the call waits for all earlier work of the device and returns
 * after the uploads and the passes have completed. */
int ptmi_scene_set_objects(ptmi_scene* s, const void* objects, uint32_t n_obj, char* err, size_t err_len);

/*
 * How each object moved between two frames, for ptmi_reproject_motion: from the previous and the current
 * object records (HOST pointers, n_obj * 1024 bytes each, the same objects in the same order) into
 * motion_dev, n_obj * PTMI_MOTION_DOUBLES doubles of device memory, 16-byte aligned.  Record k belongs to
 * object k of the caller's list -- the id of the first-hit records:
 *   [0..12)   rows 0-2 of B = prev.transform * cur.inverse: a current world point -> where that surface
 *             point was in the previous frame
 *   [12..21)  G = L(prev.inverse_transpose) * L(cur.transform)^T (L: the upper-left 3 x 3), row-major:
 *             the same map for normals (unnormalised)
 *   [21]      0.0 static: the 384 bytes of transform, inverse and inverse_transpose are equal in both
 *             records;  2.0 no history: the bottom row of cur.inverse or of prev.transform is not
 *             (0, 0, 0, 1), or an entry of B or G is not finite;  otherwise 1.0 moved
 *   [22..24)  0
 * The products are computed on the host, each entry as ((a0 b0 + a1 b1) + a2 b2) + a3 b3, separately
 * rounded (ptmi/temporal.py motion_matrices states them).  PTMI_ERR_ARG before any device call for a NULL
 * pointer, n_obj outside 1..16 or a misaligned buffer.  The copy runs in stream order; the call returns
 * when it is done (it may block the host).
 */
#define PTMI_MOTION_DOUBLES 24
int ptmi_motion_table(const void* prev_objects, const void* cur_objects, uint32_t n_obj, double* motion_dev,
                      void* hip_stream, char* err, size_t err_len);

/*
 * ptmi_reproject for scenes whose objects move (ptmi_scene_set_objects): motion_dev is the table
 * ptmi_motion_table wrote for the previous and the current frame's objects, n_obj its length (1..16).
 * Per pixel with a first hit on object k = its record's id:
 *   static (state 0), or k outside [0, n_obj): exactly ptmi_reproject's path -- with an all-static table
 *     every output equals ptmi_reproject's bit for bit;
 *   no history (state 2): the pixel resets;
 *   moved (state 1):  x' = B (x_p, 1), each row ((b0 x + b1 y) + b2 z) + b3;  m = G n_p, each row
 *     (g0 n.x + g1 n.y) + g2 n.z;  l = (m0^2 + m1^2) + m2^2, the pixel resets unless l > 0 and finite;
 *     n' = m / sqrt(l).  x' is projected with the previous camera, and the taps are tested with
 *     n' . n_q >= normal_cos and |n' . (x_q - x')| <= plane_dist * t_p.  The blend is ptmi_reproject's.
 * Rigid and affine motions of whole objects are followed.  Only what the first-hit records carry is:
 * for shadows, reflections and indirect light that move with an object see ptmi_rectify (with
 * ptmi_history_gather in this call's place), and
 * geometry inside a mesh does not deform.  The exact operation order is ptmi/temporal.py
 * reproject_reference with `motion`.  All of ptmi_reproject's rules and argument checks apply; the motion
 * table is one more input no output may overlap, and must be 16-byte aligned.
 */
int ptmi_reproject_motion(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                          const double* prev_hist_dev, const double* prev_feat_dev, const void* prev_camera,
                          uint32_t width, uint32_t height, const ptmi_reproject_params* params /* NULL = defaults */,
                          double* out_hist_dev, double* out_rgba_dev /* may be NULL */,
                          double* out_se_dev /* may be NULL */, const double* motion_dev, uint32_t n_obj,
                          void* hip_stream, char* err, size_t err_len);

/*
 * History rectification: ptmi_reproject / ptmi_reproject_motion in two steps, with a test of the history
 * against this frame between the lookup and the blend.  A history is found by geometry alone, so lighting
 * that changed (ptmi_scene_set_objects may change emission, colour and material; shadows and reflections
 * move with an object) would otherwise stay wrong for max_history frames.
 *
 * ptmi_history_gather does everything ptmi_reproject (motion_dev == NULL and n_obj == 0) or
 * ptmi_reproject_motion (a table of n_obj = 1..16 records) does up to the blend, and writes the history as
 * found: per pixel of gathered_dev (W*H*PTMI_HISTORY_DOUBLES) [0..2] h_c, [3] h_var, [4] h_N, [5..7] 0 --
 * the very values those calls blend -- and for a pixel they would reset (rgb, se^2, 0): N = 0 says that no
 * history was found.  Their rules and argument checks apply; max_history is checked and not used.
 *
 * ptmi_rectify, per pixel p with colour c_p, v_p = se_p^2, object id id_p and gathered record (h, hv, hn):
 *   RESET   c_p or se_p not finite: (c_p, v_p, N = 0);  hn == 0: (c_p, v_p, N = 1) -- ptmi_reproject's resets.
 *   WINDOW  taps q = p + (dx, dy), dy outer, dx inner, both in [-radius, radius], raster order, centre
 *           included; ACCEPTED when inside the image, id_q == id_p (a NaN id matches nothing), c_q and se_q
 *           finite and gathered_q.N > 0.  Sequential, separately rounded sums in tap order:
 *             m += 1;  a_k += c_q.k - c_p.k;  b_k += h_q.k - c_p.k;  sv += se_q^2;  sh += hv_q
 *   TEST    d_k = (b_k - a_k) / m;  d2 = (d_0^2 + d_1^2) + d_2^2;  V = (sv + sh) / (m m);  T2 = (gamma gamma) V.
 *           If m >= min_count and d2 > T2:  rho = sqrt(T2 / d2),  f = 1 - rho,  h'_k = h_k - f d_k,
 *           hn' = rho hn;  otherwise rho = 1 and h' = h, hn' = hn bit for bit (a NaN compares false: not
 *           rectified).  hv is not changed.
 *   BLEND   ptmi_reproject's: N' = min(hn' + 1, max_history), a = 1 / N', colour' = h' + a (c_p - h'),
 *           var' = (a a) v_p + ((1 - a)(1 - a)) hv.
 *   out_hist_dev = (colour', var', N', rho, 0, 0) ([5] = rho; 1.0 for a reset); out_rgba_dev and
 *   out_se_dev (each may be NULL) as ptmi_reproject's.  With min_count above (2 radius + 1)^2 the two calls
 *   give ptmi_reproject's / ptmi_reproject_motion's outputs bit for bit ([5] aside).
 * The means of the gathered history and of this frame are compared over the same pixels of one object,
 * against the variance of those two means: what varies inside the window (a penumbra, a texture) is in
 * both and cancels, a change in time is left, and about 49 pixels give the test 49 times a per-pixel
 * one's power.  The history is moved by the part of the offset that exceeds the tolerance and its length is
 * cut by the same factor, so a wrong history is also forgotten sooner.  The exact operation order is
 * ptmi/temporal.py gather_reference and rectify_reference.
 * Limits: only a change of the window MEAN is seen; a window with fewer than min_count accepted pixels
 * (thin objects, object edges) is not tested; the window's pixels are taken for independent, which a
 * bilinearly gathered history is not -- gamma absorbs that.
 * Both calls allocate nothing and are asynchronous on the stream.  No output may overlap an input
 * (gathered_dev is one) or another output; every buffer but se_dev and out_se_dev must be 16-byte aligned.
 * PTMI_ERR_ARG (no launch, no device call) as ptmi_reproject; for ptmi_history_gather also a motion table
 * without objects or objects without a table; for ptmi_rectify a radius outside 1..4, a negative or
 * non-finite gamma, max_history outside 1..65536 and non-zero flags.
 */
typedef struct ptmi_rectify_params {
    uint32_t radius;      /* window half-size, default 3 (7x7); 1..4 */
    uint32_t min_count;   /* default 9: fewer accepted taps -> no test */
    double gamma;         /* default 3.0; finite, >= 0 */
    uint32_t max_history; /* default 32; 1..65536 */
    uint32_t flags;       /* 0 */
} ptmi_rectify_params;

int ptmi_history_gather(const double* rgba_dev, const double* se_dev, const double* feat_dev,
                        const double* prev_hist_dev, const double* prev_feat_dev, const void* prev_camera,
                        uint32_t width, uint32_t height, const ptmi_reproject_params* params /* NULL = defaults */,
                        double* gathered_dev, const double* motion_dev /* NULL: static */, uint32_t n_obj,
                        void* hip_stream, char* err, size_t err_len);
int ptmi_rectify(const double* rgba_dev, const double* se_dev, const double* feat_dev, const double* gathered_dev,
                 uint32_t width, uint32_t height, const ptmi_rectify_params* params /* NULL = defaults */,
                 double* out_hist_dev, double* out_rgba_dev /* may be NULL */, double* out_se_dev /* may be NULL */,
                 void* hip_stream, char* err, size_t err_len);

/*
 * The standard error of a frame's pixels, estimated instead of taken from the frame's own samples: the one
 * input of ptmi_reproject, ptmi_reproject_motion, ptmi_history_gather + ptmi_rectify and ptmi_denoise that a
 * frame of few samples cannot give (ptmi_error_map: se = +inf at 1 spp, a sample variance that is itself
 * noise at 2-8 spp, se = 0 where the few paths all missed the light).  Pass out_se_dev to those calls in
 * the place of the rendered map; with it a sequence of 1-spp frames accumulates.  Two estimates:
 * TEMPORAL, the first and second moments of each surface point's frames, accumulated through
 * ptmi_history_gather's lookup on a moment history of this call's own (callers ping-pong two), and
 * SPATIAL, where that history is shorter than min_temporal, the variance of a window of same-surface pixels
 * of this frame.
 *
 * Moment record, per pixel of out_mom_dev (W*H*PTMI_MOMENT_DOUBLES): [0..2] mu, the accumulated mean colour;
 * [3] mu2, the accumulated mean of (r r + g g) + b b;  [4] N;  [5] the estimate's source: 0 none, 1 temporal,
 * 2 spatial, 3 fallback;  [6] the estimated variance;  [7] 0.
 * Per pixel p with colour c, s = (c_r c_r + c_g c_g) + c_b c_b and first-hit record (x_p, t_p, n_p, id_p):
 *   NOT FINITE  c not finite: the record is (c, s, N = 0, 0, 0, 0) and out_se = se_p (+inf when se_dev is
 *           NULL) -- ptmi_reproject's reset: later frames read nothing from it.
 *   GATHER  exactly ptmi_history_gather's projection, its four taps in its order and its acceptance tests
 *           (inside the image, N_q > 0 and a finite record, the same id, the normal and the plane distance;
 *           with a motion table its states 0 / 1 / 2) on prev_mom_dev and prev_feat_dev.  With W the sum of
 *           the accepted taps' bilinear weights w:
 *             h_mu.k = c_k + (sum w (mu_q.k - c_k)) / W;  h_mu2 = s + (sum w (mu2_q - s)) / W;  h_N = (sum w N_q) / W
 *           -- means weighted by w (not the sum w^2 / W^2 weights of ptmi_reproject's h_var).  The resets are the
 *           gather's: no history (prev_mom_dev NULL), a miss, a point behind the previous camera,
 *           W < min_weight or W == 0, motion state 2.
 *   BLEND   reset: mu' = c, mu2' = s, N' = 1.  Else N' = min(h_N + 1, max_history), a = 1 / N',
 *           mu'_k = h_mu.k + a (c_k - h_mu.k),  mu2' = h_mu2 + a (s - h_mu2).
 *   TEMPORAL  N' >= min_temporal:  d = mu2' - ((mu'_r mu'_r + mu'_g mu'_g) + mu'_b mu'_b),
 *           var = (d < 0 ? 0 : d) (N' / (N' - 1)),  source 1.
 *   SPATIAL otherwise: taps q = p + (dx, dy), dy outer, dx inner, both in [-radius, radius], raster order,
 *           centre included; ACCEPTED when inside the image, c_q finite and id_q == id_p (a NaN id matches
 *           nothing, misses match misses), and, when p is a hit (not id_p < 0),
 *           (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= window_normal_cos.  Sequential, separately rounded
 *           sums in tap order, D = c_q - c:   m += 1;  e_k += D_k;  b += (D_r D_r + D_g D_g) + D_b D_b.
 *           m >= min_count:  E = e / m,  d = b / m - ((E_r E_r + E_g E_g) + E_b E_b),
 *           var = (d < 0 ? 0 : d) (m / (m - 1)),  source 2.
 *   FALLBACK  otherwise, source 3:  var = se_p^2 when se_dev is given and se_p is finite, else var = s -- the
 *           pixel's own magnitude, a 100 % relative error: deliberately pessimistic.
 *   out_mom_dev = (mu', mu2', N', source, var, 0);  out_se_dev = sqrt(var): the standard error of THIS frame's
 *   pixel value, which is what every consumer of se expects.
 * A constant sequence comes back with var = 0 and mu' = c bit for bit (the forms written around c and s).  Every
 * operation is an IEEE add, multiply, divide, square root or comparison; the exact order is ptmi/temporal.py
 * variance_reference.
 * Limits: the temporal estimate includes real changes of a surface point's radiance (view-dependent shading,
 * moving lights) and the spatial one shading gradients and texture inside the window: both then overestimate,
 * which causes more filtering, not false confidence.  The moment history is not rectified.
 * Allocates nothing; asynchronous on the stream.  No output may overlap an input or another output; the ranges
 * are checked.  Every buffer but se_dev and out_se_dev must be 16-byte aligned.
 * PTMI_ERR_ARG (no launch, no device call) for a NULL required pointer (se_dev, prev_mom_dev and motion_dev may
 * be NULL; a history needs prev_feat_dev and prev_camera), zero width or height, a parameter outside its range
 * below, non-zero flags, a negative or non-finite threshold, overlapping or misaligned buffers, a prev_camera
 * that is singular, not finite or of another width or height, a motion table without objects or objects
 * without a table, and n_obj above 16.
 */
#define PTMI_MOMENT_DOUBLES 8
typedef struct ptmi_variance_params {
    uint32_t max_history;   /* default 32; 1..65536 */
    uint32_t min_temporal;  /* default 4: N' below it -> spatial estimate; 2..65536 */
    uint32_t radius;        /* spatial window half-size, default 3 (7x7); 1..4 */
    uint32_t min_count;     /* default 9: fewer accepted window taps -> fallback; >= 2 */
    uint32_t flags;         /* 0 */
    double normal_cos, plane_dist, min_weight;  /* the gather's, defaults as ptmi_reproject_params */
    double window_normal_cos;                   /* default 0.9: window taps on hit pixels need n_p.n_q >= it */
} ptmi_variance_params;

int ptmi_variance_estimate(const double* rgba_dev, const double* se_dev /* may be NULL */, const double* feat_dev,
                           const double* prev_mom_dev /* NULL: first frame */, const double* prev_feat_dev,
                           const void* prev_camera, uint32_t width, uint32_t height,
                           const ptmi_variance_params* params /* NULL = defaults */,
                           double* out_mom_dev, double* out_se_dev,
                           const double* motion_dev /* NULL: static */, uint32_t n_obj,
                           void* hip_stream, char* err, size_t err_len);

/* Kernel timing: with timing enabled, every trace_kernel launch of the scene is
 * bracketed by HIP events recorded on the launch stream; ptmi_scene_kernel_time
 * waits for them, returns the summed kernel milliseconds and launch count since
 * the last call, and resets the tally. */
int ptmi_scene_set_timing(ptmi_scene* s, int enable);
int ptmi_scene_kernel_time(ptmi_scene* s, double* total_ms, uint32_t* launches, char* err, size_t err_len);

/* Build / ABI identification (kernel name, offload arch, flags). */
const char* ptmi_build_info(void);

/* Diagnostics, host only (no device call): the traversal index ptmi_scene_create would
 * build for these records (ptmi_bvh.cpp), summarised into out[0..n_out):
 *   [0] Node4 count  [1] occupied child slots  [2] sum over occupied slots of the
 *   decoded child box's surface area, in object-space units  [3] infinite bounds among
 *   them  [4] largest root scale exponent s (bounds stored as (b - ctr) / 2^s)
 *   [5] roots  [6] longest chain of Node4s (the walk's stack holds <= 3 entries per
 *   level; ptmi_bvh.cpp keeps it <= 7)  [7] the child codes' leaf bit: 2^15 when every
 *   code fits the affine kernels' 16-bit traversal stack, else 2^30 (an affine scene then
 *   runs the wide-code instantiation, 32-bit stack).  Index quality (box inflation from the
 *   binary16 bounds) can be compared across translated or scaled copies of one mesh. */
int ptmi_index_stats(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                     const void* groups, uint32_t n_grp, const void* camera, double* out, int n_out,
                     char* err, size_t err_len);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
