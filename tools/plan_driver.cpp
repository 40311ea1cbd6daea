// DIAGNOSTIC: a stand-alone host program over the work plan (csrc/ptmi_plan.h plan_work, TileOwnership), for
// sanitizer builds -- no HIP, no Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pathtracer-ocl_amd/csrc tools/plan_driver.cpp -o /tmp/plan_driver && /tmp/plan_driver
// The extreme requests of tests/golden/work_plans.json: an empty sample range, no resident waves, a stride
// above the tile count (ranks that own nothing), 2^26 samples with and without a tile list, the refusals.  Each
// plan's owned tiles go into a heap buffer of exactly owned_tiles entries, so a write past it is caught, and
// every index is checked against the frame.
#include <cstdio>
#include <cstring>
#include <memory>

#include "ptmi_plan.h"

using namespace ptmi;

static int fail(const char* what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

static PlanRequest request(uint32_t w, uint32_t h, int flags, int waves, uint32_t samples, uint32_t begin, uint32_t end,
                           uint32_t stride, uint32_t offset, uint32_t chunks) {
    PlanRequest q;
    q.width = w, q.height = h, q.flags = flags, q.resident_waves = waves;
    q.samples = samples, q.sample_begin = begin, q.sample_end = end;
    q.tile_stride = stride, q.tile_offset = offset, q.chunks = chunks;
    return q;
}

// Plans q; returns the status, and for a plan lists its owned tiles into an exactly sized buffer.
static int run(const PlanRequest& q, const PlanKnobs& kn, PlanResult& r, int& rc) {
    char err[160] = "";
    const int status = plan_work(q, kn, r, err, sizeof err);
    if (status != kPlanOk) {
        if (!err[0]) rc |= fail("a refusal without a message");
        return status;
    }
    const uint32_t tiles = ((q.width + kTile - 1) / kTile) * ((q.height + kTile - 1) / kTile);
    if (r.wp.n_whole + r.wp.n_tail != r.owned_tiles) rc |= fail("n_whole + n_tail == owned_tiles");
    if (r.wp.order || r.wp.cost || r.wp.tiles) rc |= fail("the plan's pointers are null");
    if (!q.has_list) {
        if (r.own.count() != r.owned_tiles) rc |= fail("count() is the plan's owned_tiles");
        std::unique_ptr<uint32_t[]> owned(new uint32_t[r.owned_tiles]);
        for (uint32_t k = 0; k < r.owned_tiles; k++) owned[k] = r.own(k);
        for (uint32_t k = 0; k < r.owned_tiles; k++)
            if (owned[k] >= tiles) rc |= fail("an owned tile outside the frame");
    }
    return status;
}

int main() {
    int rc = 0;
    PlanResult r;
    PlanKnobs plain, mesh;
    mesh.min_chunk = 64;  // as upload_scene sets it for mesh scenes

    // an empty sample range: one chunk of length 1, every tile whole, no partials
    for (int flags : {0, (int)F_GROUPS, F_ALL | F_PROJ})
        for (int waves : {0, 16, 4096}) {
            if (run(request(100, 75, flags, waves, 2048, 1024, 1024, 1, 0, 0), flags ? mesh : plain, r, rc) != kPlanOk)
                rc |= fail("an empty range plans");
            if (r.wp.nchunks != 1 || r.wp.chunk_len != 1 || r.wp.n_tail != 0 || r.partial_bytes != 0)
                rc |= fail("an empty range is one chunk of whole tiles");
        }
    // no resident waves (an occupancy query that failed): still a plan that covers the range
    for (int flags : {0, (int)F_GROUPS, (int)(F_GROUPS | F_XRNG), F_ALL | F_WIDE})
        for (uint32_t stride : {1u, 2u, 3u}) {
            if (run(request(64, 48, flags, 0, 2048, 0, 2048, stride, stride - 1, 0), flags ? mesh : plain, r, rc) != kPlanOk)
                rc |= fail("no resident waves plans");
            const uint64_t sum = (uint64_t)r.wp.n_long * r.wp.chunk_len + (uint64_t)(r.wp.nchunks - r.wp.n_long) * r.wp.tail_len;
            if (sum < 2048) rc |= fail("the chunks cover the range");
        }
    // a stride above the tile count: 48 tiles over 50 ranks, raster; ranks 48 and 49 own nothing
    uint32_t owned = 0;
    for (uint32_t off = 0; off < 50; off++) {
        if (run(request(64, 48, F_GROUPS, 4096, 2048, 0, 2048, 50, off, 0), mesh, r, rc) != kPlanOk)
            rc |= fail("a stride above the tile count plans");
        if (r.own.tlist || r.owned_tiles != (off < 48 ? 1u : 0u)) rc |= fail("48 tiles over 50 ranks");
        owned += r.owned_tiles;
    }
    if (owned != 48) rc |= fail("every tile has one owner");
    // diagonal ownership: 8 tile rows of 8, stride 8; tile (x, y) to rank (x + y) mod 8
    for (uint32_t off = 0; off < 8; off++) {
        if (run(request(64, 64, F_GROUPS, 4096, 2048, 0, 2048, 8, off, 0), mesh, r, rc) != kPlanOk || !r.own.tlist ||
            !(r.kflags & F_TLIST) || r.owned_tiles != 8)
            rc |= fail("a diagonal plan");
        for (uint32_t k = 0; k < r.owned_tiles; k++)
            if ((r.own(k) % 8 + r.own(k) / 8) % 8 != off) rc |= fail("the diagonal's owner");
    }
    // 2^26 samples: the tile-list kernels' 2^25 bound makes two chunks of one; a pooled moment item is refused
    if (run(request(64, 48, F_GROUPS, 4096, 1u << 26, 0, 1u << 26, 2, 1, 1), mesh, r, rc) != kPlanOk ||
        r.wp.nchunks != 2 || r.wp.chunk_len != (1u << 25))
        rc |= fail("2^26 samples on a tile list: two chunks");
    PlanRequest q = request(64, 48, F_GROUPS, 4096, 1u << 26, 0, 1u << 26, 1, 0, 1);
    q.moments = true;
    if (run(q, mesh, r, rc) != kPlanErrArg) rc |= fail("a pooled moment item of 2^26 samples is refused");
    q.flags = F_GROUPS | F_XRNG;  // not pooled
    if (run(q, mesh, r, rc) != kPlanOk || !(r.kflags & F_MOM)) rc |= fail("the same item without the pool");
    q.flags = F_GROUPS, q.has_list = true, q.n_list = 7;  // a caller's list: F_TLIST, so two chunks
    if (run(q, mesh, r, rc) != kPlanOk || r.wp.nchunks != 2 || r.owned_tiles != 7) rc |= fail("a caller's list");
    // the split form: every tile chunked; no moment variant
    q = request(64, 48, F_GROUPS, 4096, 2048, 0, 2048, 1, 0, 0);
    q.split_chunk = 64;
    if (run(q, mesh, r, rc) != kPlanOk || !r.split || r.planes || r.wp.n_whole != 0 || r.wp.nchunks != 32)
        rc |= fail("the split form");
    q.moments = true;
    if (run(q, mesh, r, rc) != kPlanErrUnsupported) rc |= fail("the split form has no moment variant");
    // bad arguments
    if (run(request(64, 48, 0, 4096, 0, 0, 0, 1, 0, 0), plain, r, rc) != kPlanErrArg) rc |= fail("no samples");
    if (run(request(64, 48, 0, 4096, 8, 0, 8, 0, 0, 0), plain, r, rc) != kPlanErrArg) rc |= fail("stride 0");
    if (run(request(64, 48, 0, 4096, 8, 0, 8, 2, 2, 0), plain, r, rc) != kPlanErrArg) rc |= fail("offset >= stride");
    char tiny[8];
    if (plan_work(request(64, 48, 0, 4096, 8, 9, 8, 1, 0, 0), plain, r, tiny, sizeof tiny) != kPlanErrArg ||
        std::strlen(tiny) != sizeof tiny - 1)
        rc |= fail("a message cut to the caller's buffer");
    std::printf(rc ? "FAILED\n" : "ok\n");
    return rc;
}
