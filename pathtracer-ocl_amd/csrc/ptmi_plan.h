// ptmi_plan.h -- the work plan of a render (ptmi_api.cpp render_frame) as a pure function of the request and
// the scene's knobs: which tiles the rank owns, how many are whole and how many chunked, the chunks and the
// short last rounds, the launch's kernel flags.  Host only, no HIP and no ptmi_scene in it, so the CPU suite
// (ptmi_diag_work_plan_host, tests/test_work_plan.py) and a sanitizer build (tools/plan_driver.cpp) run it.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "ptmi_device.h"
#include "ptmi_flags.h"

namespace ptmi {

// Status codes of plan_work (include/ptmi.h PTMI_OK, PTMI_ERR_ARG, PTMI_ERR_UNSUPPORTED; ptmi_api.cpp checks).
constexpr int kPlanOk = 0, kPlanErrArg = -1, kPlanErrUnsupported = -4;

// The plan's tuning knobs of a scene (ptmi_diag_set_knob); the defaults are the product's.
struct PlanKnobs {
    uint32_t tail_tiles = 0;  // chunked tiles at the end of an automatic launch; 0: default (see plan_work)
    uint32_t tail_items = 6;  // chunk items per resident wave slot in the tail (scenes without meshes; see plan_work)
    uint32_t mesh_items = 32;  // chunk items per resident wave slot, mesh scenes (every tile chunked)
    uint32_t mesh_items_share = 48;  // ... in a sample-split rank's share (a sub-range of the samples)
    uint32_t min_chunk = 32;   // fewest samples per chunk item (see plan_work); mesh scenes: 64 (upload_scene)
    uint32_t tail_split = 4;   // mesh scenes: the last chunk round cut into this many (see plan_work)
    uint32_t tail_min = 0;     // ... while those keep at least this many samples; 0: automatic (see plan_work)
};

struct PlanRequest {
    uint32_t width = 0, height = 0;  // the frame
    uint32_t samples = 0, sample_begin = 0, sample_end = 0;
    uint32_t tile_stride = 1, tile_offset = 0;
    uint32_t chunks = 0;     // the caller's chunk count; 0: automatic
    bool has_list = false;   // a caller's tile list (ptmi_scene_render_tiles) of n_list tiles
    uint32_t n_list = 0;
    int flags = 0;           // the scene's kernel flags, F_XRNG included (ptmi_flags.h with_rng)
    int resident_waves = 0;  // device-wide resident waves of the scene's trace_kernel
    bool moments = false;    // second moments asked for (ptmi_scene_render_moments)
    uint32_t split_chunk = 0;  // 0: the one-kernel form; else the study build's split form, samples per pixel-chunk
};

// Tile ownership of a tile-split launch.  Raster: tiles offset, offset + stride, ...; with
// 160 tiles per row (1280 px) and stride 8 that gives every rank the same tile columns in
// every row -- vertical stripes, which split a mesh unevenly (C5 8 ranks: max/mean 1.05).
// Affine mesh scenes whose tile rows divide by the stride take the diagonal instead --
// tile (x, y) belongs to rank (x + y) mod stride, each row holding tiles_x / stride of a
// rank's tiles -- through the F_TLIST instantiations (WorkPlan::tiles), so the one-GPU
// kernels are untouched (profiles/r5/tile_skew).  Every pixel's sums are the same either way.
struct TileOwnership {
    bool tlist = false;  // diagonal: the launch takes the owned tiles as a list
    uint32_t tiles_x = 0, per_row = 0, stride = 1, offset = 0;
    uint32_t tiles = 0;  // of the frame
    // Diagonal for affine narrow-code mesh scenes in parity mode whose tile rows divide by the stride (the
    // F_TLIST instantiations), raster striding otherwise (and for the split form).  Also behind
    // ptmi_diag_tile_ownership, so callers that mask shards use the library's own decision (ADVICE r5:
    // ptmi/dist.py had restated it).
    static bool diagonal(int flags, uint32_t width, uint32_t tile_stride, bool split_form) {
        const uint32_t tx = (width + kTile - 1) / kTile;
        if (split_form) return false;
        return tile_stride > 1 && tile_list_supported(flags) && tx % tile_stride == 0;
    }
    uint32_t operator()(uint32_t k) const {  // owned tile k's raster index
        if (!tlist) return offset + k * stride;
        const uint32_t ty = k / per_row, j = k - ty * per_row;
        return ty * tiles_x + (offset + stride - ty % stride) % stride + j * stride;
    }
    uint32_t count() const { return tlist ? tiles / stride : (tiles + stride - 1 - offset) / stride; }
};

struct PlanResult {
    WorkPlan wp{};          // order, cost and tiles null: render_frame's resources
    TileOwnership own;      // of the library's own tile split (a caller's list replaces it)
    int kflags = 0;         // the launch's kernel flags: the request's, F_TLIST and F_MOM decided here
    uint32_t owned_tiles = 0;
    bool pooled = false;    // the scene's mesh kernel is the path-pool one (ptmi_flags.h pool_kernel)
    bool split = false;     // the split form runs this render
    bool planes = true;     // partial layout (ptmi_kernels.hip store_sums): r, g, b planes
    size_t partial_bytes = 0;  // of the chunk partial sums
};

inline int plan_error(int rc, char* err, size_t n, const char* fmt, ...) {
    if (err && n) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, n, fmt, ap);
        va_end(ap);
    }
    return rc;
}
inline int plan_bad_arguments(const PlanRequest& rq, char* err, size_t n) {
    return plan_error(kPlanErrArg, err, n, "bad render arguments (samples %u range [%u,%u) tiles %u/%u)", rq.samples,
                      rq.sample_begin, rq.sample_end, rq.tile_offset, rq.tile_stride);
}

// One plan for the plain and the moment render, so the moment render's colour sums are the plain render's bit
// for bit; a caller's list (tile_stride 1, tile_offset 0) is planned by the same code over its n_list tiles.
inline int plan_work(const PlanRequest& rq, const PlanKnobs& kn, PlanResult& r, char* err, size_t err_len) {
    if (rq.samples == 0 || rq.sample_begin > rq.sample_end || rq.sample_end > rq.samples || rq.tile_stride == 0 ||
        rq.tile_offset >= rq.tile_stride)
        return plan_bad_arguments(rq, err, err_len);
    const uint32_t samples = rq.samples, tile_stride = rq.tile_stride, tile_offset = rq.tile_offset;
    const uint32_t range = rq.sample_end - rq.sample_begin;
    const uint32_t tiles_x = (rq.width + kTile - 1) / kTile, tiles = tiles_x * ((rq.height + kTile - 1) / kTile);
    const int kflags0 = rq.flags;
    const bool tlist = !rq.has_list && TileOwnership::diagonal(kflags0, rq.width, tile_stride, rq.split_chunk != 0);
    r.own = TileOwnership{tlist, tiles_x, tiles_x / tile_stride, tile_stride, tile_offset, tiles};
    const uint32_t owned_tiles = rq.has_list ? rq.n_list : r.own.count();
    // Work items (WorkPlan, ptmi_device.h).  Automatic (chunks == 0), scenes without
    // meshes: whole tiles first, then the last ~0.5 resident waves' worth of tiles
    // split into sample chunks, so that short items fill the end of the launch (~6 per
    // resident wave slot, >= 32 samples each).  A whole-tile item pays its start-up
    // and the spread of its lanes' path lengths once for the whole range, and sums in
    // sample order without a partial buffer.  C2 (2048 spp, 4096 resident waves): 185.3 ms
    // with every tile chunked; 181.6 / 178.2 / 177.5 / 176.8 / 182.5 ms with 9000 / 4096 /
    // 3072 / 2048 / 1024 chunked tail tiles.
    // Round 3: ~6 items per slot, with the partials as r, g, b planes (24 B per lane and
    // item): C2 2048 spp 154.0 / 154.5 / 154.9 / 155.3 ms and 0.164 / 0.143 / 0.131 / 0.12 GB
    // of HBM traffic per launch at 8 / 6 / 5 / 4 items (profiles/r3/tail_items).
    // Mesh scenes chunk every tile (~32 items per slot): a tile's cost there depends on
    // how much mesh it sees, so whole tiles leave a long tail (C4 801 -> 1008 ms).
    // An explicit chunk count splits every tile.
    WorkPlan& wp = r.wp;
    wp = WorkPlan{};
    wp.s_begin = rq.sample_begin;
    wp.s_end = rq.sample_end;
    wp.tile_stride = tile_stride;
    wp.tile_offset = tile_offset;
    // (a caller's list: the F_TLIST instantiations where the scene's family has them, else the moment
    // instantiation's own select on WorkPlan::tiles, ptmi_kernels.hip kTilesOf)
    const int kflags = kflags0 | ((tlist || (rq.has_list && tile_list_supported(kflags0))) ? F_TLIST : 0);
    // Affine mesh scenes in parity mode, when the split form is selected (render_split): pixel-chunks of
    // split_chunk samples (an explicit `chunks` sets the chunk count as for the one-kernel
    // form, so both forms then sum the same chunks in the same order).
    const bool split = rq.split_chunk && tile_list_supported(kflags) && range > 0;
    uint32_t chunks = rq.chunks;
    if (split) {
        uint32_t nch = chunks ? chunks : (range + rq.split_chunk - 1) / rq.split_chunk;
        nch = std::max<uint32_t>(1, std::min<uint32_t>(nch, range));
        wp.chunk_len = (range + nch - 1) / nch;
        wp.nchunks = (range + wp.chunk_len - 1) / wp.chunk_len;
        wp.n_long = wp.nchunks;
        wp.tail_len = wp.chunk_len;
        wp.n_whole = 0;
        wp.n_tail = owned_tiles;
    }
    const bool mesh = (kflags0 & F_GROUPS) != 0;
    uint32_t n_tail = owned_tiles;
    const bool auto_chunks = chunks == 0;
    if (split) {
        chunks = wp.nchunks;
    } else if (chunks == 0) {
        if (!mesh || kn.tail_tiles)
            n_tail = std::min<uint32_t>(owned_tiles, kn.tail_tiles ? kn.tail_tiles : (uint32_t)(rq.resident_waves / 2));
        // A sample-split rank of a mesh scene holding at most a quarter of the samples (every tile):
        // 48 items per slot instead of 32 (round 6, C4 8 ranks: projected efficiency 0.896 -> 0.904;
        // at 2 ranks 48 cost 0.962 -> 0.940, and the one-GPU frame 1.7 %, so those keep 32).
        // Tile-split ranks keep 32 (C5: 0.857 / 0.854).
        const bool sample_share = mesh && tile_stride == 1 && (uint64_t)range * 4 <= samples;
        const uint64_t want =
            (uint64_t)rq.resident_waves * (mesh ? (sample_share ? kn.mesh_items_share : kn.mesh_items) : kn.tail_items);
        // A mesh scene's tile-split rank owns 1/N of the tiles, so a chunk round is a fraction
        // of the machine (2,400 items at N = 8 against 4,096 wave slots) and the 64-sample floor
        // held it at ~19 items per slot; half the floor lets the items-per-slot target bind
        // (C5 8 ranks: 55 chunks of 38 samples, projected efficiency 0.81 -> 0.84; C4 tile split
        // 0.80 -> 0.81).  Sample-split ranks keep every tile and the floor (C4 0.90 -> 0.86 at
        // the half floor; profiles/r5/shards/chunks).
        const uint32_t floor = (mesh && tile_stride > 1) ? std::max<uint32_t>(1, kn.min_chunk / 2) : kn.min_chunk;
        chunks = (uint32_t)std::min<uint64_t>((want + n_tail - 1) / std::max<uint32_t>(n_tail, 1),
                                              std::max<uint32_t>(range / floor, 1));
    }
    // The path pool of the tile-list kernels numbers an item's paths 64 x its samples in 32 bits.
    if (kflags & F_TLIST) chunks = std::max<uint32_t>(chunks, (range + (1u << 25) - 1) >> 25);
    chunks = std::max<uint32_t>(1, std::min<uint32_t>(chunks, std::max<uint32_t>(range, 1)));
    const uint32_t chunk_len = range == 0 ? 1 : (range + chunks - 1) / chunks;
    chunks = range == 0 ? 1 : (range + chunk_len - 1) / chunk_len;
    if (chunks == 1 && !split) n_tail = 0;  // one chunk: every tile is whole
    wp.n_whole = owned_tiles - n_tail;
    wp.n_tail = n_tail;
    wp.nchunks = chunks;
    wp.chunk_len = chunk_len;
    wp.n_long = chunks;
    wp.tail_len = chunk_len;
    // Mesh scenes, automatic plans: the last chunk round is cut into tail_split shorter rounds,
    // numbered last (and so dispatched last), so the launch drains on short items -- the
    // end-of-launch ramp was 3.1 % of the one-GPU C5 frame's slot-time (profiles/r4/timeline).
    // 2048 spp, one MI355X (profiles/r5/tail_split): C5 876 -> 865 ms, C4 unchanged.  Only
    // while the short chunks keep >= min_chunk / 2 samples: on 8-rank shares (64-sample chunks)
    // 16-sample ones cost C4's sample split more at each item's end than they saved at the
    // launch's (projected efficiency 0.893 -> 0.878) and left C5's tile split as it was.
    // Round 6: the path-pool kernels (affine mesh scenes in parity mode) have no per-item lane
    // drain, so their short chunks may go down to 8 samples (tail_min): an 8-rank C5 tile share
    // (38-sample chunks) drained 9.8 ms of its 108.9 ms on its last round's costliest tiles
    // (profiles/r6/timeline).  Chunks are summed in chunk order either way.
    const bool pooled = pool_kernel(kflags0);
    const uint32_t tail_min = kn.tail_min ? kn.tail_min : pooled ? 8u : kn.min_chunk / 2;
    const uint32_t tl = (chunk_len + std::max<uint32_t>(kn.tail_split, 1) - 1) / std::max<uint32_t>(kn.tail_split, 1);
    if (!split && auto_chunks && mesh && chunks > 1 && kn.tail_split > 1 && tl >= tail_min) {
        const uint32_t rest = range - (chunks - 1) * chunk_len;
        wp.n_long = chunks - 1;
        wp.tail_len = tl;
        wp.nchunks = wp.n_long + (rest + tl - 1) / tl;
        chunks = wp.nchunks;
    }
    if (rq.moments) {
        if (split)
            return plan_error(kPlanErrUnsupported, err, err_len, "the split execution form has no moment variant");
        // The path pool numbers an item's paths 64 x its samples in 32 bits (trace_groups_pool's
        // `total`): with or without a tile list, an item of 2^26 samples or more would wrap.
        if (pooled && (uint64_t)std::max(wp.chunk_len, wp.tail_len) >= (1ull << 26) && range > 0)
            return plan_error(kPlanErrArg, err, err_len,
                              "moment render: a pooled work item of %u samples (>= 2^26); use more chunks",
                              std::max(wp.chunk_len, wp.tail_len));
    }
    r.kflags = kflags | (rq.moments ? F_MOM : 0);
    r.owned_tiles = owned_tiles;
    r.pooled = pooled;
    r.split = split;
    r.planes = !mesh || !split;
    // (moment renders: one more plane of partials, ptmi_kernels.hip store_mom)
    r.partial_bytes = (size_t)wp.n_tail * 64 * chunks * ((r.planes ? 3 : 4) + (rq.moments ? 1 : 0)) * sizeof(double);
    return kPlanOk;
}

}  // namespace ptmi
