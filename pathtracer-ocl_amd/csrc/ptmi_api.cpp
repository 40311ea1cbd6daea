// ptmi_api.cpp -- C ABI of libptmi.so (include/ptmi.h), the part that owns a ptmi_scene: record validation and
// conversion to the HBM layout (ptmi_device.h), device residency, launch orchestration, the scene's feature
// passes, the multi-GPU driver and the diagnostics.  Replaces the reference host driver
// internal/ocl/ocltracer.go (Trace / computeBatch, ocltracer.go:98-376).  The image-space passes, which take
// no scene, are in ptmi_image_api.cpp (their argument checks: ptmi_image_args.h); what both files share
// (set_err, HIP_TRY, rd<>, convert_camera) is in ptmi_api_internal.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ptmi.h"
#include "../../include/ptmi_diag.h"
#include "ptmi_api_internal.h"
#include "ptmi_bvh.h"
#include "ptmi_camcull.h"
#include "ptmi_device.h"
#include "ptmi_f16.h"
#include "ptmi_flags.h"
#include "ptmi_motion.h"
#include "ptmi_plan.h"

// DIAGNOSTIC study build (make study): the split execution form, the standalone walk
// kernels and the measured tile order (ptmi_kernels.hip PTMI_STUDY).  The product has 0.
#ifndef PTMI_STUDY
#define PTMI_STUDY 0
#endif
#include "ptmi_launch.h"

using namespace ptmi;

static_assert(kPlanOk == PTMI_OK && kPlanErrArg == PTMI_ERR_ARG && kPlanErrUnsupported == PTMI_ERR_UNSUPPORTED,
              "ptmi_plan.h states the status codes of include/ptmi.h");

// A device allocation that a scene owns and that only grows: pointer plus capacity in bytes.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    // Room for `bytes`: nothing if it is there; else, after the stream's work on the old allocation, a new one
    // (contents are not kept).
    hipError_t reserve(size_t bytes, hipStream_t st) {
        if (bytes <= cap) return hipSuccess;
        hipError_t e = hipSuccess;
        if (p && (e = hipStreamSynchronize(st)) == hipSuccess && (e = hipFree(p)) == hipSuccess) p = nullptr, cap = 0;
        if (e == hipSuccess && (e = hipMalloc((void**)&p, bytes)) == hipSuccess) cap = bytes;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

// What mesh_tile_cost needs of a scene, kept with it so the tile classes are computed on
// the first render that orders tiles, and only for the tiles that render owns: the camera
// and, per group object, rows 0-2 of its inverse and its roots' hulls.
struct TileCostInput {
    DevCamera cam{};
    struct Obj {
        double inv[12];
        std::vector<std::array<double, 6>> hulls;  // (mn xyz, mx xyz) per root
    };
    std::vector<Obj> objs;
};

// The kernel flags of a scene (ptmi_flags.h F_*) in two parts: what the objects, the triangles, the
// traversal index and the force hook decide (SceneFlagBasis, fixed when the scene is created), and what the
// camera adds (scene_flags), so that a camera change re-derives the instantiation from the same code.
struct SceneFlagBasis {
    int obj_bits = 0;       // F_GROUPS | F_CYLCUBE | F_MATERIALS
    bool affine = true;     // every object and triangle normal passes the affine test below
    bool tris_affine = true;  // the triangles' share of `affine` (they never change on a resident scene)
    bool textured = false;  // the one textured instantiation
    int forced = -1;        // ptmi_diag_force_flags at creation (-1: none)
    int wide = 0;           // F_WIDE
};

struct ptmi_scene {
    int device = 0;
    DevScene dev{};
    void* buffers[15] = {};  // [10..12]: texture arrays, [13]: hemisphere table, [14]: camera record
    DevBuf<double> partial;     // chunk partial sums, grown on demand
    double* sunf = nullptr;     // DoF aperture table for sunf_samples (sunflower_kernel)
    uint32_t sunf_samples = 0;
    int resident_waves = 0;  // device-wide resident waves of trace_kernel
    PlanKnobs knobs;         // of the work plan (ptmi_plan.h; ptmi_diag_set_knob)
    // Mesh scenes: per-tile cost class (mesh_tile_cost) and the dispatch order built from it
    // for the last (tile_stride, tile_offset) rendered (see ensure_dispatch_order).
    // 0: raster order, 1: static (hull-hit classes), 2: measured by the last launch (needs a
    // build with PTMI_TILE_COST=1 -- see ptmi_kernels.hip item_cost_add; else the order is
    // arbitrary within the static plan, which never changes a result)
    int tile_order = 1;
    TileCostInput tc_in;              // mesh scenes: the inputs of the tile classes
    std::vector<uint8_t> tile_cost;   // per tile: its class, or kCostUnset until a render needs it
    std::vector<uint32_t> order_host;
    DevBuf<uint32_t> order_dev;
    unsigned long long* cost_dev = nullptr;  // study build: per-tile durations of the launches since the last order
    uint32_t order_stride = 0, order_offset = 0, order_n = 0, order_whole = 0;
    bool order_tlist = false;  // the dispatch order was built for a list launch
    void drop_dispatch_order() { order_n = 0; }  // the next ordered render builds it again
    void drop_tile_classes() {  // the view or the group objects changed: new classes, and the order built from them
        tile_cost.clear();
        drop_dispatch_order();
    }
    // Tile-split launches of the affine mesh kernels: the owned-tile list (WorkPlan::tiles)
    // of the last (tile_stride, tile_offset) rendered with one (see ensure_tile_list).
    std::vector<uint32_t> tlist_host;
    DevBuf<uint32_t> tlist_dev;
    uint32_t* item_ctr = nullptr;  // the mesh kernels' work-item counter (ptmi_kernels.hip take_item), zeroed per launch
    uint32_t tlist_stride = 0, tlist_offset = 0;
    uint32_t width = 0, height = 0;
    int flags = 0;  // scene features -> kernel instantiation (ptmi_flags.h F_*)
    int launch_flags() const { return with_rng(flags, rng == PTMI_RNG_XOSHIRO); }  // ... with the RNG mode's bit
    SceneFlagBasis basis;  // what `flags` takes from everything but the camera (ptmi_scene_set_camera)
    // ptmi_scene_set_objects: the converted list as uploaded (type runs, each group's RootRec slot in
    // child_base), the caller's records' identity fields, and the sizes of the two allocations that follow
    // the number of scale+translate spheres
    std::vector<DevObject> objs_host;
    std::vector<ObjectIdentity> identity;
    uint32_t n_grp = 0;
    size_t sphere_bytes = 0, cam_bytes = 0;  // allocated: buffers[6], buffers[14]
    int hemi_mismatch = 0;  // hemisphere-table records where affine and generic sequences differ (upload_scene)
    int rng = PTMI_RNG_NOISE3D;  // ptmi_scene_set_rng: PTMI_RNG_XOSHIRO launches the F_XRNG instantiations
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;  // pending (start, stop) pairs
    std::vector<hipEvent_t> spare;
#if PTMI_STUDY
    // Split execution of affine mesh scenes (ptmi_kernels.hip trace_split_kernel): a measured
    // alternative (3.3x slower than the one-kernel form on C4), study build only;
    // ptmi_diag_set_split(s, 1) selects it, ptmi_diag_set_knob tunes it.
    int split = 0;
    uint32_t split_chunk = 64;       // samples per pixel-chunk (PTMI_KNOB_SPLIT_CHUNK)
    uint32_t split_per_lane = 4;     // slots per tracer lane slot (PTMI_KNOB_SPLIT_SLOTS)
    uint32_t split_sync = 8;         // passes between completion checks (PTMI_KNOB_SPLIT_SYNC)
    uint32_t split_budget = 4;       // samples a slot starts per pass (PTMI_KNOB_SPLIT_BUDGET)
    SplitBufs sb{};
    void* split_mem = nullptr;
    size_t split_bytes = 0;
    uint32_t* split_host = nullptr;  // pinned: the request count read back at a check
    uint32_t split_passes = 0;       // passes of the last split render (diagnostics)
    uint32_t plan_split_chunk() const { return split ? split_chunk : 0; }  // PlanRequest::split_chunk
#else
    uint32_t plan_split_chunk() const { return 0; }  // the one-kernel form is the only one here
#endif
};

// ptmi_diag_force_flags: kernel flags forced onto every scene created after the call
// (-1: none).  Test hook for the generic instantiations.
static std::atomic<int> g_force_flags{-1};

namespace {

int check_device(int idx, char* err, size_t err_len) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_err(err, err_len, "no HIP device available (ptmi requires an MI355X / gfx950)");
        return PTMI_ERR_DEVICE;
    }
    if (idx < 0 || idx >= n) {
        set_err(err, err_len, "device index %d out of bounds: highest device index: %d", idx, n - 1);
        return PTMI_ERR_DEVICE;
    }
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, idx) != hipSuccess) {
        set_err(err, err_len, "hipGetDeviceProperties(%d) failed", idx);
        return PTMI_ERR_DEVICE;
    }
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0) {
        set_err(err, err_len, "device %d is %s; libptmi is built for gfx950 only", idx, p.gcnArchName);
        return PTMI_ERR_DEVICE;
    }
    return PTMI_OK;
}

// Convert + validate the packed reference records (layout.py / tracer.cl:24-93).
// Zero-pattern predicates (exact zeros, +-0 included).
bool is_st_pattern(const double* m) {  // [a 0 0 d; 0 b 0 e; 0 0 c f; 0 0 0 g]
    static const int z[] = {1, 2, 4, 6, 8, 9, 12, 13, 14};
    for (int i : z)
        if (m[i] != 0.0) return false;
    return true;
}
bool is_diag3(const double* m) {  // rows 0-2 diagonal (row 3 unused)
    static const int z[] = {1, 2, 3, 4, 6, 7, 8, 9, 11};
    for (int i : z)
        if (m[i] != 0.0) return false;
    return true;
}

// One 1024-byte CLObject record -> DevObject (everything but its place in the scene: child_base, and for
// a group the RootRec slot that replaces its roots): the one conversion behind ptmi_scene_create and
// ptmi_scene_set_objects, so both give the kernels the same bits.  A group's child_count is the record's.
int convert_object(const uint8_t* b, uint32_t i, uint32_t n_grp, DevObject& o, char* err, size_t err_len) {
    std::memset(&o, 0, sizeof o);
    o.key = (int32_t)i;
    std::memcpy(o.inv, b + 128, 128);
    std::memcpy(o.inv_t, b + 256, 128);
    std::memcpy(o.color, b + 384, 32);
    std::memcpy(o.emission, b + 416, 32);
    o.refractive_index = rd<double>(b + 448);
    const int64_t type = rd<int64_t>(b + 456);
    o.type = (type >= 0 && type <= 4) ? (int32_t)type : 999;
    o.min_y = rd<double>(b + 464);
    o.max_y = rd<double>(b + 472);
    o.reflectivity = rd<double>(b + 480);
    std::memcpy(o.bb_min, b + 520, 32);
    o.st = is_st_pattern(o.inv) ? 1 : 0;
    o.invt_diag = is_diag3(o.inv_t) ? 1 : 0;
    std::memcpy(o.bb_max, b + 552, 32);
    o.tex = b[844] ? 1 : 0;  // isTextured, textureIndex, isTexturedNM, textureIndexNM (ocltracer.go:44-47)
    o.tex_index = b[845];
    o.tex_nm = b[846] ? 1 : 0;
    o.tex_index_nm = b[847];
    std::memcpy(o.tex_scale, b + 488, 32);  // textureScaleX, Y, XNM, YNM (ocltracer.go:36-39)
    o.child_count = 0;
    if (o.type == 4) {
        const int32_t cc = rd<int32_t>(b + 584);
        if (cc < 0 || cc > 64) {
            set_err(err, err_len, "object %u: childCount %d out of range", i, cc);
            return PTMI_ERR_ARG;
        }
        for (int32_t c = 0; c < cc; c++) {
            const int32_t r = rd<int32_t>(b + 588 + 4 * c);
            if (r < 0 || (uint32_t)r >= n_grp) {
                set_err(err, err_len, "object %u: child root %d outside %u groups", i, r, n_grp);
                return PTMI_ERR_ARG;
            }
        }
        o.child_count = cc;
    }
    return PTMI_OK;
}

// Intersectable objects in type runs [planes | spheres | cylinders | cubes |
// groups], list order inside a run.  Types > 4 and groups without BVH roots
// can never record an intersection (tracer.cl:551-720) and are left out.
void sort_into_runs(const std::vector<DevObject>& all, std::vector<DevObject>& objs, int32_t run_end[5]) {
    objs.clear();
    for (int t = 0; t < 5; t++) {
        for (const DevObject& o : all)
            if (o.type == t && (t != 4 || o.child_count > 0)) objs.push_back(o);
        run_end[t] = (int32_t)objs.size();
    }
}

int convert_scene(const uint8_t* objects, uint32_t n_obj, const uint8_t* tris, uint32_t n_tri, const uint8_t* groups,
                  uint32_t n_grp, const uint8_t* camera, std::vector<DevObject>& objs, std::vector<int32_t>& roots,
                  std::vector<DevNode>& nodes, RootIndex& index, std::vector<RootRec>& root_rec,
                  std::vector<DevTriShade>& st, DevCamera& cam, int32_t run_end[5], char* err, size_t err_len) {
    if (!objects || n_obj == 0 || n_obj > PTMI_MAX_OBJECTS) {
        set_err(err, err_len, "need 1..%d objects (tracer.cl:846 __local object objects[16]), got %u",
                PTMI_MAX_OBJECTS, n_obj);
        return PTMI_ERR_ARG;
    }
    if (!camera || (n_tri && !tris) || (n_grp && !groups)) {
        set_err(err, err_len, "NULL record pointer");
        return PTMI_ERR_ARG;
    }
    if (const int rc = convert_camera(camera, cam, err, err_len)) return rc;
    std::vector<DevObject> all(n_obj);
    for (uint32_t i = 0; i < n_obj; i++) {
        const uint8_t* b = objects + (size_t)PTMI_OBJECT_BYTES * i;
        DevObject& o = all[i];
        if (const int rc = convert_object(b, i, n_grp, o, err, err_len)) return rc;
        o.child_base = (int32_t)roots.size();
        for (int32_t c = 0; c < o.child_count; c++) roots.push_back(rd<int32_t>(b + 588 + 4 * c));
    }
    sort_into_runs(all, objs, run_end);
    nodes.resize(n_grp);
    std::vector<int32_t> tri_off(n_grp), tri_cnt(n_grp);
    for (uint32_t g = 0; g < n_grp; g++) {
        const uint8_t* b = groups + (size_t)PTMI_GROUP_BYTES * g;
        DevNode& n = nodes[g];
        std::memcpy(n.bb_min, b + 0, 24);
        std::memcpy(n.bb_max, b + 32, 24);
        tri_off[g] = rd<int32_t>(b + 128);
        tri_cnt[g] = rd<int32_t>(b + 132);
        n.child0 = rd<int32_t>(b + 140);
        n.child1 = rd<int32_t>(b + 144);
        if (tri_cnt[g] < 0 || tri_off[g] < 0 || (int64_t)tri_off[g] + tri_cnt[g] > (int64_t)n_tri ||
            n.child0 >= (int32_t)n_grp || n.child1 >= (int32_t)n_grp) {
            set_err(err, err_len, "group %u: triangle range [%d,+%d) / children (%d,%d) out of range", g,
                    tri_off[g], tri_cnt[g], n.child0, n.child1);
            return PTMI_ERR_ARG;
        }
    }
    // Children must follow their parent (BuildCLGroup preorder numbering): the
    // trees are then acyclic and every walk terminates.
    for (int32_t g = 0; g < (int32_t)n_grp; g++)
        if ((nodes[g].child0 > 0 && nodes[g].child0 <= g) || (nodes[g].child1 > 0 && nodes[g].child1 <= g)) {
            set_err(err, err_len, "group %d: child index not in preorder (BuildCLGroup numbering)", g);
            return PTMI_ERR_ARG;
        }
    st.resize(n_tri);
    for (uint32_t t = 0; t < n_tri; t++) {
        const uint8_t* b = tris + (size_t)PTMI_TRIANGLE_BYTES * t;
        std::memcpy(st[t].n1, b + 160, 32);
        std::memcpy(st[t].n2, b + 192, 32);
        std::memcpy(st[t].n3, b + 224, 32);
        std::memcpy(st[t].color, b + 256, 32);
    }
    // Per group object: one traversal index over all its roots' triangles
    // (ptmi_bvh.cpp); the object then refers to its RootRec (child_count 1).
    index = RootIndex{};
    root_rec.clear();
    for (DevObject& o : objs) {
        if (o.type != 4) continue;
        RootRec rec;
        const int rc = build_object_index(tris, nodes, tri_off, tri_cnt, roots.data() + o.child_base, o.child_count,
                                          o.bb_min, o.bb_max, index, &rec, err, err_len);
        if (rc) return rc;
        o.child_base = (int32_t)root_rec.size();
        o.child_count = 1;
        root_rec.push_back(rec);
    }
    return PTMI_OK;
}

template <typename T>
int upload(const std::vector<T>& v, void** dst, char* err, size_t err_len) {
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 256);
    HIP_TRY(hipMalloc(dst, bytes));
    if (!v.empty()) HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PTMI_OK;
}


// The affine instantiations also use the compiler's divide / sqrt cores for sphere
// roots (ptmi_kernels.hip div_core), which needs 2a = 2|M d|^2
// far above the denormal range for every unit-scale ray direction d: each sphere's
// inverse has linear-part entries <= 2^64 and |det| >= 2^-64, so its smallest singular
// value is >= 2^-196.  Scenes outside that take the generic instantiation.
// The same bound on the camera inverse keeps |pixel - origin| >= 2^-196 for its
// normalize's core, and on sphere inverses (through their transposes) keeps sphere
// normals >= 2^-196 long.
bool tame(const double* m) {
    double mx = 0.0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) mx = std::max(mx, std::fabs(m[4 * r + c]));
    const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) +
                       m[2] * (m[4] * m[9] - m[5] * m[8]);
    return mx <= 0x1p64 && std::fabs(det) >= 0x1p-64;
}

// Affine camera (ptmi_kernels.hip dotv): the inverse ends in (+-0, +-0, +-0, 1) and is tame.
bool camera_affine(const DevCamera& cam) {
    return cam.inv[12] == 0.0 && cam.inv[13] == 0.0 && cam.inv[14] == 0.0 && cam.inv[15] == 1.0 && tame(cam.inv);
}

int scene_flags(const SceneFlagBasis& fb, const DevCamera& cam) {
    int flags = fb.obj_bits;
    if (cam.aperture != 0) flags |= F_DOF;
    // Affine scene: every inverse ends in (+-0, +-0, +-0, 1), inverse transposes have +-0 in
    // column 3 of rows 0-2, triangle normals have a finite w.  Otherwise F_PROJ: the generic
    // instantiation with the w lanes.
    if (!(fb.affine && camera_affine(cam))) flags |= F_PROJ;
    if (fb.textured) flags = F_GENERIC;
    if (fb.forced >= 0) flags = fb.forced & F_GENERIC;
    return flags | fb.wide;  // (never a 16-bit stack for 31-bit codes: F_PROJ and F_TEX kernels have 32-bit ones)
}

// A scene converted on the host once (records validated and split into the device
// layouts, traversal indices built, kernel flags chosen), uploadable to any device.
struct HostScene {
    std::vector<DevObject> objs;
    std::vector<int32_t> roots;
    std::vector<DevNode> nodes;
    RootIndex index;
    std::vector<RootRec> root_rec;
    std::vector<DevTriShade> st;
    std::vector<PlaneRec> planes;
    std::vector<SphereRec> spheres;
    DevCamera cam{};
    int32_t run_end[5] = {};
    int flags = 0;
    SceneFlagBasis basis;
    int32_t leaf_bit = kLeafNarrow;  // Node4 child code format (finalize_index_codes)
    uint32_t n_list = 0, n_grp = 0, n_tri = 0;
    int32_t n_planes_y = 0;
    std::vector<ObjectIdentity> identity;  // per record of the caller's list (ptmi_scene_set_objects)
};

// What the flags take from the objects (the converted list) and the triangles: obj_bits, affine, textured.
// The one derivation behind ptmi_scene_create and ptmi_scene_set_objects.
void object_flag_basis(const std::vector<DevObject>& objs, bool tris_affine, SceneFlagBasis& fb) {
    fb.obj_bits = 0;
    fb.affine = true;
    fb.textured = false;
    for (const DevObject& o : objs) {
        if (o.type == 4) fb.obj_bits |= F_GROUPS;
        if (o.type == 2 || o.type == 3) fb.obj_bits |= F_CYLCUBE;
        if (o.reflectivity != 0.0 || o.refractive_index != 1.0) fb.obj_bits |= F_MATERIALS;
    }
    for (const DevObject& o : objs)
        fb.affine = fb.affine && o.inv[12] == 0.0 && o.inv[13] == 0.0 && o.inv[14] == 0.0 && o.inv[15] == 1.0 &&
                    o.inv_t[3] == 0.0 && o.inv_t[7] == 0.0 && o.inv_t[11] == 0.0;
    fb.affine = fb.affine && tris_affine;
    for (const DevObject& o : objs)
        if (o.type == 1) fb.affine = fb.affine && tame(o.inv);
    // Textured plane/sphere/cube colours or plane normal maps: the one textured
    // instantiation (generic arithmetic + software sampler, tracer.cl:907-914, 1077-1092).
    for (const DevObject& o : objs)
        if ((o.tex && (o.type == 0 || o.type == 1 || o.type == 3)) || (o.tex_nm && o.type == 0)) fb.textured = true;
}

// The compact plane / scale+translate sphere records (ptmi_device.h) of a converted object list, with
// the planes' pairing: likewise shared by create and update.
void compact_records(const std::vector<DevObject>& objs, std::vector<PlaneRec>& planes, std::vector<SphereRec>& spheres,
                     int32_t& n_planes_y) {
    planes.clear();
    spheres.clear();
    for (size_t k = 0; k < objs.size(); k++) {
        const DevObject& o = objs[k];
        if (o.type == 0) {
            PlaneRec r{};
            std::memcpy(r.row1, o.inv + 4, 32);
            r.slot = (int32_t)k;
            r.key = o.key;
            r.nz = (r.row1[0] != 0.0 ? 1 : 0) | (r.row1[1] != 0.0 ? 2 : 0) | (r.row1[2] != 0.0 ? 4 : 0);
            planes.push_back(r);
        } else if (o.type == 1 && o.st) {
            SphereRec r{};
            r.m0 = o.inv[0];
            r.m3 = o.inv[3];
            r.m5 = o.inv[5];
            r.m7 = o.inv[7];
            r.m10 = o.inv[10];
            r.m11 = o.inv[11];
            r.m15 = o.inv[15];
            r.slot = (int32_t)k;
            r.key = o.key;
            spheres.push_back(r);
        }
    }
    // The leading planes (list order kept) whose row 1 has +-0 x and z entries, and the
    // parallel pairs (identical row1[0..2]) as the affine plane loops pair the planes:
    // (0,1), (2,3), ... below n_planes_y, then on from there (find_closest_prims).
    const int np = (int)planes.size();
    int npy = 0;
    while (npy < np && planes[npy].row1[0] == 0.0 && planes[npy].row1[2] == 0.0) npy++;
    n_planes_y = npy;
    auto same = [&](int a, int b) { return std::memcmp(planes[a].row1, planes[b].row1, 24) == 0; };
    int p = 0;
    for (; p + 1 < npy; p += 2) planes[p].par = same(p, p + 1);
    for (; p + 1 < np; p += 2) planes[p].par = same(p, p + 1);
}

int prepare_scene(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri, const void* groups,
                  uint32_t n_grp, const void* camera, const ptmi_textures* textures, HostScene& hs, char* err,
                  size_t err_len) {
    int rc = convert_scene((const uint8_t*)objects, n_obj, (const uint8_t*)triangles, n_tri, (const uint8_t*)groups,
                           n_grp, (const uint8_t*)camera, hs.objs, hs.roots, hs.nodes, hs.index, hs.root_rec, hs.st,
                           hs.cam, hs.run_end, err, err_len);
    if (rc) return rc;
    hs.leaf_bit = finalize_index_codes(hs.index, hs.root_rec);
    // What the flags take from the objects, the triangles and the force hook (SceneFlagBasis); the camera's
    // part is scene_flags', which ptmi_scene_set_camera runs again, the objects' part object_flag_basis',
    // which ptmi_scene_set_objects runs again.
    SceneFlagBasis& fb = hs.basis;
    fb = SceneFlagBasis{};
    for (const DevTriShade& t : hs.st)
        fb.tris_affine = fb.tris_affine && std::isfinite(t.n1[3]) && std::isfinite(t.n2[3]) && std::isfinite(t.n3[3]);
    object_flag_basis(hs.objs, fb.tris_affine, fb);
    // Child codes past 16 bits (>= 2^15 Node4s or triangles): a traversal stack of 32-bit
    // entries -- the affine F_WIDE instantiation (ptmi_kernels.hip trace_groups), or the
    // generic one for non-affine scenes (round 5 sent every such scene to the generic one).
    fb.wide = hs.leaf_bit != kLeafNarrow ? F_WIDE : 0;
    fb.forced = g_force_flags.load();  // ptmi_diag_force_flags (tests): one load
    const int flags = scene_flags(fb, hs.cam);
    if (textures) {
        for (int k = 0; k < 3; k++) {
            const uint64_t texels = (uint64_t)textures->width[k] * textures->height[k] * textures->count[k];
            if (textures->count[k] &&
                (!textures->pixels[k] || textures->width[k] == 0 || textures->height[k] == 0 ||
                 textures->width[k] > (1u << 16) || textures->height[k] > (1u << 16) || textures->count[k] > 256 ||
                 texels > ((uint64_t)1 << 32))) {
                set_err(err, err_len, "texture array %d: bad size %ux%u x %u layers (or NULL pixels)", k,
                        textures->width[k], textures->height[k], textures->count[k]);
                return PTMI_ERR_ARG;
            }
        }
    }
    hs.flags = flags;
    compact_records(hs.objs, hs.planes, hs.spheres, hs.n_planes_y);
    hs.identity.resize(n_obj);
    for (uint32_t i = 0; i < n_obj; i++)
        hs.identity[i] = object_identity((const uint8_t*)objects + (size_t)PTMI_OBJECT_BYTES * i);
    hs.n_list = n_obj;
    hs.n_grp = n_grp;
    hs.n_tri = n_tri;
    return PTMI_OK;
}

// Device-wide resident tile waves of the scene's trace_kernel instantiation (its work
// plan is sized by them, ptmi_scene_render).
hipError_t resident_waves(ptmi_scene* s) {
    hipDeviceProp_t p;
    hipError_t e = hipGetDeviceProperties(&p, s->device);
    if (e != hipSuccess) return e;
    const int flags = s->launch_flags();
    s->resident_waves = p.multiProcessorCount * 16;
    int blocks_per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, trace_kernel_symbol(flags),
                                                     trace_block_threads(flags), 0) == hipSuccess &&
        blocks_per_cu > 0)
        s->resident_waves = p.multiProcessorCount * blocks_per_cu * trace_tiles_per_block(flags);
    return hipSuccess;
}

// Mesh scenes: a cost class per 8x8 tile for the dispatch order of the chunked tiles --
// how many of 9 primary rays (a 3x3 grid of pixel centres) pass the conservative hull
// cull of some group object (group_needs_walk without the primitives' best).  Tiles whose
// camera rays reach a mesh walk on every bounce; their chunks are the long items of a
// launch (C4 at 2048 spp: 20 ms on average, up to 82 ms), and in raster order the last
// round of chunks ends on them (a 43 ms drain, 6 % of the slot-time; tools/timeline.py).
// Dispatching them first within each chunk round leaves short items for the end.  Only the
// order of work items changes, never a pixel's sums or their order.  Plain host doubles: a
// heuristic, not an exactness argument.
constexpr uint8_t kCostUnset = 0xFF;

// The mesh kernels' walk batch for a scene (DevScene::walk_batch): larger meshes have longer walks
// (gopher: 9.8 Node4 visits and 5.3 triangle tests per walk against the teapot's 6.7 and 2.3), so
// a walk phase is worth more parked lanes.  Scenes without meshes never walk.
static int32_t walk_batch_for(const HostScene& hs) {
    if (!(hs.flags & F_GROUPS)) return 64;
    return hs.n_tri >= 12000 ? 32 : 28;
}

TileCostInput tile_cost_input(const HostScene& hs) {
    TileCostInput in;
    in.cam = hs.cam;
    for (int j = hs.run_end[3]; j < hs.run_end[4]; j++) {
        const DevObject& ob = hs.objs[j];
        TileCostInput::Obj o;
        std::memcpy(o.inv, ob.inv, sizeof(o.inv));
        for (int ci = 0; ci < ob.child_count; ci++) {
            const RootRec& R = hs.root_rec[ob.child_base + ci];
            o.hulls.push_back({R.hull_mn[0], R.hull_mn[1], R.hull_mn[2], R.hull_mx[0], R.hull_mx[1], R.hull_mx[2]});
        }
        in.objs.push_back(std::move(o));
    }
    return in;
}

// The class of tile t (raster index).
uint8_t mesh_tile_class(const TileCostInput& in, const std::vector<std::array<double, 3>>& org, int t) {
    const DevCamera& c = in.cam;
    const int tx = (c.width + 7) / 8;
    const double* m = c.inv;
    int hits = 0;
    for (int q = 0; q < 9; q++) {
        const double x = (t % tx) * 8 + 1 + 3 * (q % 3) + 0.5, y = (t / tx) * 8 + 1 + 3 * (q / 3) + 0.5;
        const double a = c.half_width - c.pixel_size * x, b = c.half_height - c.pixel_size * y;
        double d[3];
        for (int r = 0; r < 3; r++) d[r] = m[4 * r] * a + m[4 * r + 1] * b - m[4 * r + 2] + m[4 * r + 3] - c.origin[r];
        bool hit = false;
        for (size_t j = 0; j < in.objs.size() && !hit; j++) {
            const TileCostInput::Obj& ob = in.objs[j];
            double inv_d[3];
            for (int r = 0; r < 3; r++) {
                const double* mi = ob.inv + 4 * r;
                inv_d[r] = 1.0 / (mi[0] * d[0] + mi[1] * d[1] + mi[2] * d[2]);
            }
            for (const auto& H : ob.hulls) {
                double tn = 0.0, tf = INFINITY;
                for (int r = 0; r < 3; r++) {
                    const double t0 = (H[r] - org[j][r]) * inv_d[r], t1 = (H[3 + r] - org[j][r]) * inv_d[r];
                    tn = std::max(tn, std::min(t0, t1));
                    tf = std::min(tf, std::max(t0, t1));
                }
                if (tn <= tf) {  // NaN slabs (ray in a hull face plane) count as misses: a heuristic
                    hit = true;
                    break;
                }
            }
        }
        hits += hit ? 1 : 0;
    }
    return (uint8_t)hits;
}

// Classes of the tiles owned(0), owned(1), ... owned(n - 1) not computed yet, into cost
// (sized to the frame's tiles, kCostUnset where unknown).  The camera origin in each group
// object's space is computed once per call, not per ray.
template <typename Owned>
void mesh_tile_cost(const TileCostInput& in, std::vector<uint8_t>& cost, uint32_t n, Owned owned) {
    const DevCamera& c = in.cam;
    const size_t tiles = (size_t)((c.width + 7) / 8) * ((c.height + 7) / 8);
    if (cost.size() != tiles) cost.assign(tiles, kCostUnset);
    std::vector<std::array<double, 3>> org(in.objs.size());
    for (size_t j = 0; j < in.objs.size(); j++)
        for (int r = 0; r < 3; r++) {
            const double* mi = in.objs[j].inv + 4 * r;
            org[j][r] = mi[0] * c.origin[0] + mi[1] * c.origin[1] + mi[2] * c.origin[2] + mi[3];
        }
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t t = owned(k);
        if (cost[t] == kCostUnset) cost[t] = mesh_tile_class(in, org, (int)t);
    }
}

int upload_scene(const HostScene& hs, int device_index, const ptmi_textures* textures, ptmi_scene** out, char* err,
                 size_t err_len) {
    HIP_TRY(hipSetDevice(device_index));
    ptmi_scene* s = new ptmi_scene();
    s->flags = hs.flags;
    s->basis = hs.basis;
    s->device = device_index;
    s->width = (uint32_t)hs.cam.width;
    s->height = (uint32_t)hs.cam.height;
    int rc;
    if ((rc = upload(hs.objs, &s->buffers[0], err, err_len)) || (rc = upload(hs.roots, &s->buffers[1], err, err_len)) ||
        (rc = upload(hs.nodes, &s->buffers[2], err, err_len)) ||
        (rc = upload(hs.index.tris, &s->buffers[3], err, err_len)) || (rc = upload(hs.st, &s->buffers[4], err, err_len)) ||
        (rc = upload(hs.planes, &s->buffers[5], err, err_len)) ||
        (rc = upload(hs.spheres, &s->buffers[6], err, err_len)) ||
        (rc = upload(hs.index.nodes, &s->buffers[7], err, err_len)) ||
        (rc = upload(hs.index.chain_boxes, &s->buffers[8], err, err_len)) ||
        (rc = upload(hs.root_rec, &s->buffers[9], err, err_len))) {
        ptmi_scene_destroy(s);
        return rc;
    }
    for (int k = 0; k < 3; k++) {  // texture arrays (prepareTextures, ocltracer.go:228-254)
        DevTexArray& T = s->dev.tex[k];
        T = DevTexArray{};
        if (!textures || textures->count[k] == 0) continue;  // the all-zero fake image
        const size_t bytes = (size_t)textures->width[k] * textures->height[k] * textures->count[k] * 4;
        hipError_t e = hipMalloc(&s->buffers[10 + k], bytes);
        if (e == hipSuccess) e = hipMemcpy(s->buffers[10 + k], textures->pixels[k], bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_err(err, err_len, "texture array %d upload (%zu B): %s", k, bytes, hipGetErrorString(e));
            ptmi_scene_destroy(s);
            return PTMI_ERR_HIP;
        }
        T.texels = (const uint32_t*)s->buffers[10 + k];
        T.w = (int32_t)textures->width[k];
        T.h = (int32_t)textures->height[k];
        T.layers = (int32_t)textures->count[k];
    }
    s->objs_host = hs.objs;
    s->identity = hs.identity;
    s->n_grp = hs.n_grp;
    s->sphere_bytes = std::max<size_t>(hs.spheres.size() * sizeof(SphereRec), 256);  // as upload() sized it
    s->dev.objs = (const DevObject*)s->buffers[0];
    for (int t = 0; t < 5; t++) s->dev.run_end[t] = hs.run_end[t];
    s->dev.planes = (const PlaneRec*)s->buffers[5];
    s->dev.n_planes = (int32_t)hs.planes.size();
    s->dev.n_planes_y = hs.n_planes_y;
    s->dev.spheres = (const SphereRec*)s->buffers[6];
    s->dev.n_spheres_st = (int32_t)hs.spheres.size();
    // HIP failures from here on release the half-built scene.
#define SCENE_TRY(call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            set_err(err, err_len, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                                     \
            ptmi_scene_destroy(s);                                                                 \
            return PTMI_ERR_HIP;                                                                   \
        }                                                                                          \
    } while (0)
    if (!hs.objs.empty()) {
        SCENE_TRY(launch_plane_normals((DevObject*)s->buffers[0], (int)hs.objs.size(), nullptr));
        SCENE_TRY(hipDeviceSynchronize());
    }
    {  // randomVectorInHemisphere table (ptmi_kernels.hip hemi_table_kernel) + its check counter
        const size_t tab = (size_t)65536 * 4 * sizeof(double);
        SCENE_TRY(hipMalloc(&s->buffers[13], tab + 256));
        int* mismatch = (int*)((char*)s->buffers[13] + tab);
        SCENE_TRY(hipMemset(mismatch, 0, sizeof(int)));
        SCENE_TRY(launch_hemi_table((double*)s->buffers[13], mismatch, nullptr));
        // Only the affine instantiations read the table (ptmi_kernels.hip bounce_shade), and
        // its records are the affine sequences' own results, so a record where the generic
        // (full-operator) sequences give other bits -- a toolchain or ocml change -- affects
        // no image: it is counted and reported, not a scene failure.
        SCENE_TRY(hipMemcpy(&s->hemi_mismatch, mismatch, sizeof(int), hipMemcpyDeviceToHost));
        // (ptmi_diag_hemi_mismatch returns the count; tests/test_gpu_rng.py expects 0.)
        if (s->hemi_mismatch && getenv("PTMI_VERBOSE"))
            fprintf(stderr, "ptmi: hemisphere table: %d records where the affine and generic sequences differ "
                            "(generic instantiations compute, they never read the table)\n", s->hemi_mismatch);
        s->dev.hemi = (const double*)s->buffers[13];
    }
    s->dev.roots = (const int32_t*)s->buffers[1];
    s->dev.nodes = (const DevNode*)s->buffers[2];
    s->dev.tris = (const DevTri*)s->buffers[3];
    s->dev.tri_shade = (const DevTriShade*)s->buffers[4];
    s->dev.nodes4 = (const Node4*)s->buffers[7];
    s->dev.chains = (const ChainBox*)s->buffers[8];
    s->dev.root_rec = (const RootRec*)s->buffers[9];
    s->dev.n_obj = (uint32_t)hs.objs.size();
    s->dev.n_list = hs.n_list;
    s->dev.n_nodes = hs.n_grp;
    s->dev.n_nodes4 = (int32_t)hs.index.nodes.size();
    s->dev.leaf_bit = hs.leaf_bit;
    // Walk batch of the mesh kernels (parked lanes that start a wave's walk phase; ptmi_kernels.hip
    // trace_groups / trace_groups_pool): a walk phase lasts as long as its longest walk, so the
    // batch trades the parked lanes' waiting against the phases' idle lanes.  Round 6, with the
    // path pool (2048 spp, one MI355X, profiles/r6/tune): teapot (C4) 24 / 28 / 32 -> 490.5 / 489.4 /
    // 493.6 ms, gopher (C5) 784.2 / 768.2 / 759.6 ms.
    s->dev.walk_batch = walk_batch_for(hs);
    // The hemisphere table in the mesh kernels: the 1-MB (sin, cos) plane shares each XCD's 4-MB L2
    // with the traversal index.  Round 6, with the path pool, on the gopher (C5, index ~3.7 MB) the
    // table costs HBM traffic -- 2.1-2.25 GB per launch with it, 0.76 GB without (profiles/r6/hbm1):
    // its lines are evicted and refetched -- but it still saves time: 753.3 / 754.2 / 755.2 ms with,
    // 766.7 / 767.7 / 768.3 ms without, alternated on one box (profiles/r6/hm2); the teapot (C4)
    // 488.5-490.0 with, 503.1 ms without.  At ~3 GB/s the traffic binds nothing, so every mesh scene
    // reads the table; PTMI_KNOB_HEMI_MESH 0 trades the 1.7 % for the traffic.
    s->dev.hemi_mesh = 1;
    // (Tests and tuning studies change the plan through ptmi_diag_set_knob; the library reads
    // no tuning variable from the environment.)
    // Mesh scenes: >= 64 samples per chunk.  It binds only on short sample ranges (a rank's
    // share): the C4 8-rank shares (256 samples) take 81.3 ms on average with 4 chunks of 64
    // against 85.4 ms with 7 of 37 (the items' start-up and end-of-item idle lanes), 93.5 ms
    // with 2 of 128 (a coarser drain); the C5 tile-split shares are flat (profiles/r4/shards).
    if (hs.flags & F_GROUPS) s->knobs.min_chunk = 64;
    if (hs.flags & F_GROUPS) s->tc_in = tile_cost_input(hs);  // tile classes: on the first ordered render
    s->dev.n_tri = hs.n_tri;
    s->dev.cam = hs.cam;
    {  // the camera record in device memory (ptmi_kernels.hip camera_ptr)
        // and, behind it, the camera terms of this scene's planes and spheres (ptmi_device.h), computed
        // from the record just uploaded: they go with every upload of the camera record
        s->cam_bytes = cam_record_bytes(s->dev.n_planes, s->dev.n_spheres_st, hs.cam.width, hs.cam.height);
        SCENE_TRY(hipMalloc(&s->buffers[14], s->cam_bytes));
        SCENE_TRY(hipMemcpy(s->buffers[14], &hs.cam, sizeof(DevCamera), hipMemcpyHostToDevice));
        s->dev.camg = (const DevCamera*)s->buffers[14];
        SCENE_TRY(launch_camera_terms(s->dev, nullptr));
        SCENE_TRY(hipDeviceSynchronize());
    }
    SCENE_TRY(resident_waves(s));
#undef SCENE_TRY
    *out = s;
    return PTMI_OK;
}


#if PTMI_STUDY
// Split execution of an affine mesh scene (ptmi_kernels.hip trace_split_kernel): pixel-chunks
// of chunk_len samples over every owned tile, traced pass by pass by a pool of L path slots
// (L = the tracer's resident lanes x split_per_lane), each pass followed by the walks it
// asked for, until a pass asks for none.  Chunk records go to `part` in the WorkPlan's
// chunk-major layout (store_sums' records), summed by reduce_chunks_kernel as for the
// one-kernel form's chunk items.
int render_split(ptmi_scene* s, uint32_t samples, const WorkPlan& wp, const double* seeds, double* sums,
                 hipStream_t st, char* err, size_t err_len) {
    const int flags = s->flags;
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, s->device));
    int per_cu = 0, walk_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trace_split_symbol(flags), 64, 0));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&walk_cu, walk_split_symbol(), 64, 0));
    const uint32_t waves = (uint32_t)std::max(1, per_cu) * (uint32_t)p.multiProcessorCount;
    const uint32_t walk_grid = (uint32_t)std::max(1, walk_cu) * (uint32_t)p.multiProcessorCount;
    const uint32_t per_wave = 64u * s->split_per_lane;
    const uint64_t n_items64 = (uint64_t)wp.n_tail * 64u * wp.nchunks;
    if (n_items64 >= 0xFFFFFFF0ull) {
        set_err(err, err_len, "split render: %llu pixel-chunks exceed 32-bit ids", (unsigned long long)n_items64);
        return PTMI_ERR_UNSUPPORTED;
    }
    const uint32_t n_items = (uint32_t)n_items64;
    // Slots: the tracer's resident waves x per_wave, but no more than there are pixel-chunks.
    uint32_t L = waves * per_wave;
    L = std::max<uint32_t>(64, std::min<uint32_t>(L, (n_items + 63) / 64 * 64));
    const uint32_t n_waves = (L + per_wave - 1) / per_wave;
    const size_t need = (size_t)L * (kSlotBytes + 4) + (size_t)n_waves * 12 + 512;
    if (need > s->split_bytes) {
        if (s->split_mem) {
            HIP_TRY(hipStreamSynchronize(st));
            HIP_TRY(hipFree(s->split_mem));
            s->split_mem = nullptr;
            s->split_bytes = 0;
        }
        HIP_TRY(hipMalloc(&s->split_mem, need));
        s->split_bytes = need;
    }
    if (!s->split_host) HIP_TRY(hipHostMalloc((void**)&s->split_host, 64, hipHostMallocDefault));
    char* m = (char*)s->split_mem;
    SplitBufs& B = s->sb;
    B.rec = m;
    m += (size_t)L * kSlotBytes;
    B.req = (uint32_t*)m;
    m += (size_t)L * 4;
    B.seg = (uint32_t*)m;
    m += (size_t)n_waves * 4;
    B.wcl = (uint32_t*)m;
    m += (size_t)n_waves * 8;
    B.cnt = (uint32_t*)m;
    B.L = L;
    B.per_wave = per_wave;
    B.n_items = n_items;
    B.budget = s->split_budget;
    HIP_TRY(hipMemset2DAsync(B.rec + offsetof(SplitRec, u), kSlotBytes, 0xFF, 4, L, st));  // every slot kSlotFree
    HIP_TRY(hipMemsetAsync(B.cnt, 0, 16, st));
    HIP_TRY(hipMemsetAsync(B.wcl, 0, (size_t)n_waves * 8, st));  // no block claimed yet
    // A bound no render reaches: every pass finishes or advances at least one pixel-chunk
    // by a bounce, so a runaway loop means a bug; fail instead of spinning.
    const uint64_t max_passes = ((uint64_t)n_items / L + 1) * 11ull * wp.chunk_len + 1024;
    uint32_t pass = 0;
    for (;;) {
        HIP_TRY(hipMemsetAsync(B.cnt, 0, 4, st));  // this pass's request count
        HIP_TRY(hipMemsetAsync(B.cnt + 2, 0, 4, st));  // and yield count
        HIP_TRY(launch_split_pass(s->dev, flags, samples, wp, B, seeds, s->sunf, s->partial.p, walk_grid, st));
        pass++;
        if (pass % s->split_sync == 0) {
            HIP_TRY(hipMemcpyAsync(s->split_host, B.cnt, 12, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (s->split_host[0] == 0 && s->split_host[2] == 0 && s->split_host[1] >= n_items) break;
        }
        if (pass > max_passes) {
            set_err(err, err_len, "split render did not finish in %u passes", pass);
            return PTMI_ERR_HIP;
        }
    }
    s->split_passes = pass;
    if (getenv("PTMI_SPLIT_DEBUG")) {  // (study build) slot states after the last pass
        std::vector<uint32_t> it(L);
        HIP_TRY(hipMemcpy2D(it.data(), 4, B.rec + offsetof(SplitRec, u), kSlotBytes, 4, L, hipMemcpyDeviceToHost));
        uint32_t cnt[4];
        HIP_TRY(hipMemcpy(cnt, B.cnt, 16, hipMemcpyDeviceToHost));
        size_t fr = 0, dead = 0, busy = 0;
        for (uint32_t v : it) (v == kSlotFree ? fr : v == kSlotDead ? dead : busy)++;
        fprintf(stderr, "split: L %u items %u passes %u walk_grid %u per_cu %d: free %zu dead %zu busy %zu req %u claims %u walks %u\n",
                L, n_items, pass, walk_grid, per_cu, fr, dead, busy, cnt[0], cnt[1], cnt[3]);
    }
    (void)sums;
    return PTMI_OK;
}
#endif  // PTMI_STUDY

}  // namespace

extern "C" {

int ptmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ptmi_device_name(int device_index, char* buf, size_t len) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device_index) != hipSuccess) return PTMI_ERR_DEVICE;
    if (buf && len) snprintf(buf, len, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return PTMI_OK;
}

const char* ptmi_build_info(void) {
    return "ptmi abi=1 arch=gfx950 fp=fp64 contract=off kernels=trace_kernel<F>,reduce_chunks_kernel,finalize_kernel";
}

int ptmi_index_stats(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri, const void* groups,
                     uint32_t n_grp, const void* camera, double* out, int n_out, char* err, size_t err_len) {
    if (!out || n_out <= 0) {
        set_err(err, err_len, "out == NULL");
        return PTMI_ERR_ARG;
    }
    HostScene hs;
    int rc = prepare_scene(objects, n_obj, triangles, n_tri, groups, n_grp, camera, nullptr, hs, err, err_len);
    if (rc) return rc;
    double st[8] = {(double)hs.index.nodes.size(), 0.0, 0.0, 0.0, 0.0, (double)hs.root_rec.size(), 0.0,
                    (double)hs.leaf_bit};
    for (const RootRec& R : hs.root_rec) {
        st[4] = std::max(st[4], std::log2((double)R.sc));
        std::vector<std::pair<int32_t, int>> todo;  // (Node4, its level)
        const int32_t lb = hs.leaf_bit, empty = lb | ((int32_t)hs.index.tris.size() - 1);  // the sentinel leaf
        if (R.entry < lb) todo.push_back({R.entry, 1});
        while (!todo.empty()) {  // the root's Node4s (children >= 0 are Node4 indices)
            const auto [ni, lv] = todo.back();
            const Node4& nd = hs.index.nodes[ni];
            todo.pop_back();
            st[6] = std::max(st[6], (double)lv);
            for (int i = 0; i < 4; i++) {
                if (nd.child[i] == empty) continue;
                if (nd.child[i] < lb) todo.push_back({nd.child[i], lv + 1});
                double e[3];
                for (int k = 0; k < 3; k++) {
                    const double lo = f16_value(nd.bnd[k][0][i]), hi = f16_value(nd.bnd[k][1][i]);
                    st[3] += (std::isinf(lo) ? 1 : 0) + (std::isinf(hi) ? 1 : 0);
                    e[k] = (hi - lo) * R.sc;
                }
                st[1] += 1.0;
                st[2] += 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]);
            }
        }
    }
    for (int i = 0; i < n_out && i < 8; i++) out[i] = st[i];
    return PTMI_OK;
}

int ptmi_scene_create(int device_index, const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                      const void* groups, uint32_t n_grp, const void* camera, ptmi_scene** out, char* err,
                      size_t err_len) {
    return ptmi_scene_create_textured(device_index, objects, n_obj, triangles, n_tri, groups, n_grp, camera, nullptr,
                                      out, err, err_len);
}

int ptmi_scene_create_textured(int device_index, const void* objects, uint32_t n_obj, const void* triangles,
                               uint32_t n_tri, const void* groups, uint32_t n_grp, const void* camera,
                               const ptmi_textures* textures, ptmi_scene** out, char* err, size_t err_len) {
    if (!out) {
        set_err(err, err_len, "out == NULL");
        return PTMI_ERR_ARG;
    }
    *out = nullptr;
    if (device_index < 0) device_index = 0;  // ocltracer.go:138-140
    int rc = check_device(device_index, err, err_len);
    if (rc) return rc;
    HostScene hs;
    if ((rc = prepare_scene(objects, n_obj, triangles, n_tri, groups, n_grp, camera, textures, hs, err, err_len)))
        return rc;
    return upload_scene(hs, device_index, textures, out, err, err_len);
}

void ptmi_scene_destroy(ptmi_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (void* b : s->buffers)
        if (b) (void)hipFree(b);
    s->partial.release();
    s->order_dev.release();
    s->tlist_dev.release();
    if (s->sunf) (void)hipFree(s->sunf);
#if PTMI_STUDY
    if (s->split_mem) (void)hipFree(s->split_mem);
    if (s->split_host) (void)hipHostFree(s->split_host);
#endif
    if (s->item_ctr) (void)hipFree(s->item_ctr);
    if (s->cost_dev) (void)hipFree(s->cost_dev);
    for (auto& e : s->events) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    for (auto e : s->spare) (void)hipEventDestroy(e);
    delete s;
}

int ptmi_scene_size(const ptmi_scene* s, uint32_t* w, uint32_t* h) {
    if (!s) return PTMI_ERR_ARG;
    if (w) *w = s->width;
    if (h) *h = s->height;
    return PTMI_OK;
}

}  // extern "C"

// The steps of render_frame that keep a resource of the scene in step with the plan (ptmi_plan.h).

// The diagonal owned-tile list (WorkPlan::tiles) of a tile-split launch that takes one.
static int ensure_tile_list(ptmi_scene* s, PlanResult& plan, hipStream_t st, char* err, size_t err_len) {
    const TileOwnership& own = plan.own;
    if (!own.tlist) return PTMI_OK;
    const uint32_t n = plan.owned_tiles;
    if (s->tlist_stride != own.stride || s->tlist_offset != own.offset || s->tlist_host.size() != n) {
        HIP_TRY(hipStreamSynchronize(st));  // tlist_host may still feed an earlier copy
        s->tlist_host.resize(n);
        for (uint32_t k = 0; k < n; k++) s->tlist_host[k] = own(k);
        HIP_TRY(s->tlist_dev.reserve((size_t)n * sizeof(uint32_t), st));
        HIP_TRY(hipMemcpyAsync(s->tlist_dev.p, s->tlist_host.data(), (size_t)n * sizeof(uint32_t),
                               hipMemcpyHostToDevice, st));
        s->tlist_stride = own.stride;
        s->tlist_offset = own.offset;
        s->drop_dispatch_order();  // it indexes owned tiles
    }
    plan.wp.tiles = s->tlist_dev.p;
    return PTMI_OK;
}

// Mesh scenes: the dispatch order of the work items (WorkPlan::order) -- whole tiles among themselves,
// then each chunk round's tiles among themselves (which tiles are whole and which
// chunked stays the raster-defined plan, so no pixel's sums change).  A rank's
// first launch (or one after its tile ownership or plan changed) takes the static
// order (mesh_tile_cost's hull-hit classes, costliest first, raster order within a
// class); with tile_order 2 every launch also measures its items and
// tile_order_kernel writes the next launch's order from those durations.  (The
// kernels without meshes do not measure: see item_cost_add.)
static int ensure_dispatch_order(ptmi_scene* s, PlanResult& plan, hipStream_t st, char* err, size_t err_len) {
    const TileOwnership& own = plan.own;
    WorkPlan& wp = plan.wp;
    const uint32_t n = plan.owned_tiles;
    if (plan.split || !s->tile_order || n == 0 || !(s->flags & F_GROUPS)) return PTMI_OK;
#if PTMI_STUDY
    if (s->tile_order == 2 && !s->cost_dev) {
        HIP_TRY(hipMalloc((void**)&s->cost_dev, (size_t)own.tiles * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(s->cost_dev, 0, (size_t)own.tiles * sizeof(unsigned long long), st));
    }
#endif
    if (s->order_stride != own.stride || s->order_offset != own.offset || s->order_n != n ||
        s->order_tlist != own.tlist || s->order_whole != wp.n_whole) {
        HIP_TRY(hipStreamSynchronize(st));  // order_host may still feed an earlier copy
        mesh_tile_cost(s->tc_in, s->tile_cost, n, own);  // this render's tiles, once
        s->order_host.resize(n);
        for (uint32_t k = 0; k < wp.n_whole; k++) s->order_host[k] = k;
        for (uint32_t k = 0; k < wp.n_tail; k++) s->order_host[wp.n_whole + k] = k;
        std::stable_sort(s->order_host.begin() + wp.n_whole, s->order_host.end(), [&](uint32_t a, uint32_t b) {
            return s->tile_cost[own(wp.n_whole + a)] > s->tile_cost[own(wp.n_whole + b)];
        });
        HIP_TRY(s->order_dev.reserve((size_t)n * sizeof(uint32_t), st));
        HIP_TRY(hipMemcpyAsync(s->order_dev.p, s->order_host.data(), (size_t)n * sizeof(uint32_t),
                               hipMemcpyHostToDevice, st));
        s->order_stride = own.stride;
        s->order_offset = own.offset;
        s->order_n = n;
        s->order_tlist = own.tlist;
        s->order_whole = wp.n_whole;
    }
    wp.order = s->order_dev.p;
#if PTMI_STUDY
    wp.cost = s->tile_order == 2 ? s->cost_dev : nullptr;
#endif
    return PTMI_OK;
}

// The DoF aperture table of a frame of `samples` samples (sunflower_kernel).
static int ensure_dof_table(ptmi_scene* s, uint32_t samples, hipStream_t st, char* err, size_t err_len) {
    if (!(s->flags & F_DOF) || s->dev.cam.aperture == 0 || s->sunf_samples == samples) return PTMI_OK;
    if (s->sunf) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipFree(s->sunf));
        s->sunf = nullptr;
    }
    HIP_TRY(hipMalloc((void**)&s->sunf, (size_t)samples * 2 * sizeof(double)));
    HIP_TRY(launch_sunflower(s->sunf, samples, st));
    s->sunf_samples = samples;
    return PTMI_OK;
}

// A (start, stop) event pair for a timed launch, from the scene's spares.
static int take_events(ptmi_scene* s, hipEvent_t& ev0, hipEvent_t& ev1, char* err, size_t err_len) {
    for (hipEvent_t* e : {&ev0, &ev1}) {
        if (!s->spare.empty()) {
            *e = s->spare.back();
            s->spare.pop_back();
        } else {
            HIP_TRY(hipEventCreate(e));
        }
    }
    return PTMI_OK;
}

// ptmi_scene_render (sq_dev == nullptr) and ptmi_scene_render_moments (sq_dev: W*H second moments):
// one plan for both, so the moment render's colour sums are the plain render's bit for bit.
// list_dev (ptmi_scene_render_tiles; tile_stride 1, tile_offset 0, sq_dev set): the owned tiles are the
// caller's n_list device-resident raster indices instead, planned by the same code.
static int render_frame(ptmi_scene* s, uint32_t samples, uint32_t sample_begin, uint32_t sample_end,
                        uint32_t tile_stride, uint32_t tile_offset, const double* seeds_dev, double* sums_dev,
                        double* sq_dev, uint32_t chunks, void* hip_stream, char* err, size_t err_len,
                        const uint32_t* list_dev = nullptr, uint32_t n_list = 0) {
    PlanRequest rq;
    rq.samples = samples, rq.sample_begin = sample_begin, rq.sample_end = sample_end;
    rq.tile_stride = tile_stride, rq.tile_offset = tile_offset;
    if (!s || !seeds_dev || !sums_dev) return plan_bad_arguments(rq, err, err_len);
    rq.width = s->width, rq.height = s->height;
    rq.chunks = chunks;
    rq.has_list = list_dev != nullptr, rq.n_list = n_list;
    rq.flags = s->launch_flags();
    rq.resident_waves = s->resident_waves;
    rq.moments = sq_dev != nullptr;
    rq.split_chunk = s->plan_split_chunk();
    PlanResult plan;
    int rc = plan_work(rq, s->knobs, plan, err, err_len);
    if (rc) return rc;
    const WorkPlan& wp = plan.wp;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = ensure_tile_list(s, plan, st, err, err_len))) return rc;
    // A caller's list lives on the device: the library's cached diagonal list and its cached
    // dispatch order (both built on the host from its own ownership) are left alone, and the items
    // run in list order.  (A costliest-first order of listed tiles would need the list on the host.)
    if (list_dev) plan.wp.tiles = list_dev;
    else if ((rc = ensure_dispatch_order(s, plan, st, err, err_len))) return rc;
    if ((rc = ensure_dof_table(s, samples, st, err, err_len))) return rc;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (s->timing && (rc = take_events(s, ev0, ev1, err, err_len))) return rc;
    const size_t npix = (size_t)s->width * s->height;
    const bool partial_frame = tile_stride > 1 || list_dev;  // un-owned tiles
    if (partial_frame) HIP_TRY(hipMemsetAsync(sums_dev, 0, npix * 4 * sizeof(double), st));
    if (partial_frame && sq_dev) HIP_TRY(hipMemsetAsync(sq_dev, 0, npix * sizeof(double), st));
    HIP_TRY(s->partial.reserve(plan.partial_bytes, st));
    if (!plan.split) {  // the launch's work-item counter, zeroed outside the timed span
        if (!s->item_ctr) HIP_TRY(hipMalloc((void**)&s->item_ctr, 256));
        HIP_TRY(hipMemsetAsync(s->item_ctr, 0, sizeof(uint32_t), st));
    }
    if (ev0) HIP_TRY(hipEventRecord(ev0, st));
#if PTMI_STUDY
    if (plan.split) {
        if ((rc = render_split(s, samples, wp, seeds_dev, sums_dev, st, err, err_len))) return rc;
    } else
#endif
    {
        HIP_TRY(launch_trace(s->dev, plan.kflags, samples, wp, seeds_dev, s->sunf, sums_dev, s->partial.p, s->item_ctr,
                             sq_dev, st));
    }
    if (ev1) {
        HIP_TRY(hipEventRecord(ev1, st));
        s->events.emplace_back(ev0, ev1);
    }
#if PTMI_STUDY
    // after the timed launch: the next launch's order from this one's item durations
    if (wp.cost)
        HIP_TRY(launch_tile_order(wp.cost, wp.n_whole, wp.n_tail, tile_stride, tile_offset, s->order_dev.p, st));
#endif
    HIP_TRY(launch_reduce(s->partial.p, sums_dev, wp, (int)s->width, (int)s->height, plan.planes, sq_dev, st));
    return PTMI_OK;
}

extern "C" {

int ptmi_scene_render(ptmi_scene* s, uint32_t samples, uint32_t sample_begin, uint32_t sample_end,
                      uint32_t tile_stride, uint32_t tile_offset, const double* seeds_dev, double* sums_dev,
                      uint32_t chunks, void* hip_stream, char* err, size_t err_len) {
    return render_frame(s, samples, sample_begin, sample_end, tile_stride, tile_offset, seeds_dev, sums_dev, nullptr,
                        chunks, hip_stream, err, err_len);
}

int ptmi_scene_render_moments(ptmi_scene* s, uint32_t samples, uint32_t sample_begin, uint32_t sample_end,
                              uint32_t tile_stride, uint32_t tile_offset, const double* seeds_dev, double* sums_dev,
                              double* sq_dev, uint32_t chunks, void* hip_stream, char* err, size_t err_len) {
    if (!sq_dev) {
        set_err(err, err_len, "ptmi_scene_render_moments: sq_dev == NULL");
        return PTMI_ERR_ARG;
    }
    return render_frame(s, samples, sample_begin, sample_end, tile_stride, tile_offset, seeds_dev, sums_dev, sq_dev,
                        chunks, hip_stream, err, err_len);
}

int ptmi_scene_render_tiles(ptmi_scene* s, uint32_t samples, uint32_t sample_begin, uint32_t sample_end,
                            const uint32_t* tiles_dev, uint32_t n_tiles, const double* seeds_dev, double* sums_dev,
                            double* sq_dev, uint32_t chunks, void* hip_stream, char* err, size_t err_len) {
    if (!s || !sums_dev || !sq_dev || (!tiles_dev && n_tiles > 0)) {
        set_err(err, err_len, "ptmi_scene_render_tiles: scene, sums_dev or sq_dev == NULL, or %u tiles without a list",
                n_tiles);
        return PTMI_ERR_ARG;
    }
    if (n_tiles == 0) {  // no tile owned: the two frames are zero, and no plan is made
        if (!seeds_dev || samples == 0 || sample_begin > sample_end || sample_end > samples) {
            set_err(err, err_len, "bad render arguments (samples %u range [%u,%u))", samples, sample_begin, sample_end);
            return PTMI_ERR_ARG;
        }
        HIP_TRY(hipSetDevice(s->device));
        const size_t npix = (size_t)s->width * s->height;
        HIP_TRY(hipMemsetAsync(sums_dev, 0, npix * 4 * sizeof(double), (hipStream_t)hip_stream));
        HIP_TRY(hipMemsetAsync(sq_dev, 0, npix * sizeof(double), (hipStream_t)hip_stream));
        return PTMI_OK;
    }
#if PTMI_STUDY
    if (s->split) {
        set_err(err, err_len, "the split execution form takes no tile list");
        return PTMI_ERR_UNSUPPORTED;
    }
#endif
    return render_frame(s, samples, sample_begin, sample_end, 1, 0, seeds_dev, sums_dev, sq_dev, chunks, hip_stream,
                        err, err_len, tiles_dev, n_tiles);
}

int ptmi_scene_features(ptmi_scene* s, double* feat_dev, void* hip_stream, char* err, size_t err_len) {
    if (!s || !feat_dev || ((uintptr_t)feat_dev & 15u)) {
        set_err(err, err_len, "bad feature-pass arguments");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_features(s->dev, feat_dev, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_scene_features_chain(ptmi_scene* s, double* feat_dev, uint32_t max_chain, double reflect_min,
                              void* hip_stream, char* err, size_t err_len) {
    if (!s || !feat_dev || ((uintptr_t)feat_dev & 15u)) {
        set_err(err, err_len, "bad feature-pass arguments");
        return PTMI_ERR_ARG;
    }
    if (max_chain < 1 || max_chain > 16 || !(reflect_min > 0.0 && reflect_min <= 1.0)) {  // (a NaN fails both)
        set_err(err, err_len, "bad specular-chain parameters (max_chain %u, 1..16; reflect_min %g, (0, 1])", max_chain,
                reflect_min);
        return PTMI_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_features_chain(s->dev, feat_dev, max_chain, reflect_min, (hipStream_t)hip_stream));
    return PTMI_OK;
}

int ptmi_scene_set_rng(ptmi_scene* s, int mode, char* err, size_t err_len) {
    if (!s || (mode != PTMI_RNG_NOISE3D && mode != PTMI_RNG_XOSHIRO)) {
        set_err(err, err_len, "ptmi_scene_set_rng: bad scene or mode %d", mode);
        return PTMI_ERR_ARG;
    }
    if (mode == PTMI_RNG_XOSHIRO && (s->flags & (F_PROJ | F_TEX))) {
        set_err(err, err_len, "the statistical RNG mode exists for affine, untextured scenes only (this scene is %s)",
                (s->flags & F_TEX) ? "textured" : "not affine");
        return PTMI_ERR_UNSUPPORTED;
    }
    s->rng = mode;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(resident_waves(s));
    return PTMI_OK;
}

int ptmi_scene_set_camera(ptmi_scene* s, const void* camera, char* err, size_t err_len) {
    if (!s || !camera) {
        set_err(err, err_len, "ptmi_scene_set_camera: scene or camera == NULL");
        return PTMI_ERR_ARG;
    }
    // Everything is checked before anything changes: after an error the scene renders as before.
    DevCamera cam{};
    if (const int rc = convert_camera((const uint8_t*)camera, cam, err, err_len)) return rc;
    if ((uint32_t)cam.width != s->width || (uint32_t)cam.height != s->height) {
        set_err(err, err_len, "ptmi_scene_set_camera: a %dx%d camera on a %ux%u scene (buffers and work plans keep their size)",
                cam.width, cam.height, s->width, s->height);
        return PTMI_ERR_ARG;
    }
    const int flags = scene_flags(s->basis, cam);
    if (s->rng == PTMI_RNG_XOSHIRO && (flags & (F_PROJ | F_TEX))) {  // as ptmi_scene_set_rng
        set_err(err, err_len, "the statistical RNG mode exists for affine scenes only (this camera is not affine)");
        return PTMI_ERR_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // renders in flight read the record and its terms in device memory
    HIP_TRY(hipMemcpy(s->buffers[14], &cam, sizeof(DevCamera), hipMemcpyHostToDevice));
    s->dev.cam = cam;
    s->flags = flags;
    // the camera terms go with every upload of the camera record (upload_scene)
    HIP_TRY(launch_camera_terms(s->dev, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(resident_waves(s));  // the instantiation may have changed (F_DOF, F_PROJ): the work plan's size
    if (s->flags & F_GROUPS) {  // mesh scenes: the tile classes are the view's
        s->tc_in.cam = cam;
        s->drop_tile_classes();
    }
    return PTMI_OK;
}

int ptmi_scene_set_objects(ptmi_scene* s, const void* objects, uint32_t n_obj, char* err, size_t err_len) {
    if (!s || !objects) {
        set_err(err, err_len, "ptmi_scene_set_objects: scene or objects == NULL");
        return PTMI_ERR_ARG;
    }
    // Everything is checked before anything changes: after an error the scene renders as before.
    if (n_obj != s->identity.size()) {
        set_err(err, err_len, "ptmi_scene_set_objects: %u objects on a scene of %zu (the list keeps its length)", n_obj,
                s->identity.size());
        return PTMI_ERR_ARG;
    }
    const uint8_t* recs = (const uint8_t*)objects;
    std::vector<DevObject> all(n_obj), objs;
    for (uint32_t i = 0; i < n_obj; i++) {
        const uint8_t* b = recs + (size_t)PTMI_OBJECT_BYTES * i;
        if (const char* what = identity_change(s->identity[i], object_identity(b))) {
            set_err(err, err_len, "ptmi_scene_set_objects: object %u changes its %s (the traversal index and the "
                                  "object runs were built from it: create a new scene)", i, what);
            return PTMI_ERR_ARG;
        }
        if (const int rc = convert_object(b, i, s->n_grp, all[i], err, err_len)) return rc;
    }
    int32_t run_end[5];
    sort_into_runs(all, objs, run_end);
    // equal types and child counts give the slots of the resident list: each keeps its place in the scene
    if (objs.size() != s->objs_host.size()) {
        set_err(err, err_len, "ptmi_scene_set_objects: %zu intersectable objects, the scene has %zu", objs.size(),
                s->objs_host.size());
        return PTMI_ERR_ARG;
    }
    for (size_t k = 0; k < objs.size(); k++) {
        if (objs[k].key != s->objs_host[k].key || objs[k].type != s->objs_host[k].type) {
            set_err(err, err_len, "ptmi_scene_set_objects: slot %zu holds another object", k);
            return PTMI_ERR_ARG;
        }
        objs[k].child_base = s->objs_host[k].child_base;    // groups: the RootRec slot
        objs[k].child_count = s->objs_host[k].child_count;  // (1 for a group, see convert_scene)
    }
    SceneFlagBasis basis = s->basis;  // (forced, wide and the triangles' share stay)
    object_flag_basis(objs, basis.tris_affine, basis);
    const int flags = scene_flags(basis, s->dev.cam);
    if (s->rng == PTMI_RNG_XOSHIRO && (flags & (F_PROJ | F_TEX))) {  // as ptmi_scene_set_rng
        set_err(err, err_len, "the statistical RNG mode exists for affine, untextured scenes only (these objects make "
                              "the scene %s)", (flags & F_TEX) ? "textured" : "not affine");
        return PTMI_ERR_UNSUPPORTED;
    }
    std::vector<PlaneRec> planes;
    std::vector<SphereRec> spheres;
    int32_t n_planes_y = 0;
    compact_records(objs, planes, spheres, n_planes_y);
    if ((int32_t)planes.size() != s->dev.n_planes) {  // (the types are the scene's: cannot happen)
        set_err(err, err_len, "ptmi_scene_set_objects: %zu planes, the scene has %d", planes.size(), s->dev.n_planes);
        return PTMI_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // renders in flight read the records in device memory
    // The scale+translate sphere records and the camera allocation (its terms and masks follow the
    // record) grow with the number of such spheres: a sphere that loses a rotation adds one.
    const size_t sphere_bytes = spheres.size() * sizeof(SphereRec);
    if (sphere_bytes > s->sphere_bytes) {
        void* grown = nullptr;
        HIP_TRY(hipMalloc(&grown, sphere_bytes));
        (void)hipFree(s->buffers[6]);
        s->buffers[6] = grown;
        s->sphere_bytes = sphere_bytes;
        s->dev.spheres = (const SphereRec*)grown;
    }
    const size_t cam_bytes = cam_record_bytes(s->dev.n_planes, (int32_t)spheres.size(), s->dev.cam.width, s->dev.cam.height);
    if (cam_bytes > s->cam_bytes) {
        void* grown = nullptr;
        HIP_TRY(hipMalloc(&grown, cam_bytes));
        (void)hipFree(s->buffers[14]);
        s->buffers[14] = grown;
        s->cam_bytes = cam_bytes;
        s->dev.camg = (const DevCamera*)grown;
        HIP_TRY(hipMemcpy(s->buffers[14], &s->dev.cam, sizeof(DevCamera), hipMemcpyHostToDevice));
    }
    if (!objs.empty()) {
        HIP_TRY(hipMemcpy(s->buffers[0], objs.data(), objs.size() * sizeof(DevObject), hipMemcpyHostToDevice));
        HIP_TRY(launch_plane_normals((DevObject*)s->buffers[0], (int)objs.size(), nullptr));
    }
    if (!planes.empty())
        HIP_TRY(hipMemcpy(s->buffers[5], planes.data(), planes.size() * sizeof(PlaneRec), hipMemcpyHostToDevice));
    if (!spheres.empty()) HIP_TRY(hipMemcpy(s->buffers[6], spheres.data(), sphere_bytes, hipMemcpyHostToDevice));
    s->dev.n_planes_y = n_planes_y;
    s->dev.n_spheres_st = (int32_t)spheres.size();
    s->objs_host = objs;
    s->basis = basis;
    s->flags = flags;
    // the camera terms and the tiles' candidate masks: from the records just uploaded
    HIP_TRY(launch_camera_terms(s->dev, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(resident_waves(s));  // the instantiation may have changed (F_MATERIALS, F_PROJ, F_TEX)
    if (s->flags & F_GROUPS) {  // mesh scenes: the group objects' inverses behind the tile classes
        size_t j = 0;
        for (int k = run_end[3]; k < run_end[4] && j < s->tc_in.objs.size(); k++, j++)
            std::memcpy(s->tc_in.objs[j].inv, objs[k].inv, sizeof(s->tc_in.objs[j].inv));
        s->drop_tile_classes();
    }
    return PTMI_OK;
}

int ptmi_scene_set_timing(ptmi_scene* s, int enable) {
    if (!s) return PTMI_ERR_ARG;
    s->timing = enable != 0;
    return PTMI_OK;
}

int ptmi_scene_kernel_time(ptmi_scene* s, double* total_ms, uint32_t* launches, char* err, size_t err_len) {
    if (!s) {
        set_err(err, err_len, "scene == NULL");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    double tot = 0.0;
    for (auto& e : s->events) {
        HIP_TRY(hipEventSynchronize(e.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
        tot += ms;
        s->spare.push_back(e.first);
        s->spare.push_back(e.second);
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (uint32_t)s->events.size();
    s->events.clear();
    return PTMI_OK;
}

int ptmi_trace(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri, const void* groups,
               uint32_t n_grp, int device_index, uint32_t samples, const void* camera, const double* seeds,
               uint64_t seed_stream, const ptmi_textures* textures, double* out_rgba, char* err, size_t err_len) {
    if (!out_rgba || samples == 0) {
        set_err(err, err_len, "out_rgba == NULL or samples == 0");
        return PTMI_ERR_ARG;
    }
    ptmi_scene* s = nullptr;
    int rc = ptmi_scene_create_textured(device_index, objects, n_obj, triangles, n_tri, groups, n_grp, camera,
                                        textures, &s, err, err_len);
    if (rc) return rc;
    const uint32_t npix = s->width * s->height;
    double *d_seeds = nullptr, *d_sums = nullptr;
    hipStream_t st = nullptr;
    auto fail = [&](int code) {
        if (st) (void)hipStreamDestroy(st);
        if (d_seeds) (void)hipFree(d_seeds);
        if (d_sums) (void)hipFree(d_sums);
        ptmi_scene_destroy(s);
        return code;
    };
#define TRY_OR_FAIL(call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            set_err(err, err_len, "%s failed: %s", #call, hipGetErrorString(e_));                 \
            return fail(PTMI_ERR_HIP);                                                            \
        }                                                                                         \
    } while (0)
    TRY_OR_FAIL(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    TRY_OR_FAIL(hipMalloc((void**)&d_seeds, (size_t)npix * sizeof(double)));
    TRY_OR_FAIL(hipMalloc((void**)&d_sums, (size_t)npix * 4 * sizeof(double)));
    if (seeds) {
        TRY_OR_FAIL(hipMemcpyAsync(d_seeds, seeds, (size_t)npix * sizeof(double), hipMemcpyHostToDevice, st));
    } else if ((rc = ptmi_fill_seeds(d_seeds, npix, seed_stream, st, err, err_len))) {
        return fail(rc);
    }
    if ((rc = ptmi_scene_render(s, samples, 0, samples, 1, 0, d_seeds, d_sums, 0, st, err, err_len))) return fail(rc);
    if ((rc = ptmi_finalize(d_sums, d_sums, npix, samples, st, err, err_len))) return fail(rc);
    TRY_OR_FAIL(hipMemcpyAsync(out_rgba, d_sums, (size_t)npix * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    TRY_OR_FAIL(hipStreamSynchronize(st));
#undef TRY_OR_FAIL
    fail(PTMI_OK);
    return PTMI_OK;
}

}  // extern "C"


// Sample split by cost, not count: the first sample index of device g of n (g = n ->
// samples).  Samples past n ~ 553 / ~731 put the hemisphere / anti-aliasing noise on
// the large-argument sin reduction and cost ~1 / ~2 % more (x100 weights 100, 101, 102; round 6,
// re-measured on the round-6 kernel's 8-rank shares -- round 5's 50 / 51 / 52 left rank 0 2.5 %
// over the mean).  Same table as ptmi/dist.py's sample_split_point.
static uint32_t split_point(int g, int n, uint32_t samples) {
    static const uint64_t knot[2] = {553, 731}, w[3] = {100, 101, 102};
    auto cost = [&](uint64_t m) {
        return w[0] * std::min<uint64_t>(m, knot[0]) + w[1] * (std::min<uint64_t>(std::max<uint64_t>(m, knot[0]), knot[1]) - knot[0]) +
               w[2] * (std::max<uint64_t>(m, knot[1]) - knot[1]);
    };
    const uint64_t target = ((uint64_t)g * cost(samples) + (uint64_t)n - 1) / (uint64_t)n;
    uint64_t m;
    if (target <= w[0] * knot[0])
        m = (target + w[0] - 1) / w[0];
    else if (target <= cost(knot[1]))
        m = knot[0] + (target - cost(knot[0]) + w[1] - 1) / w[1];
    else
        m = knot[1] + (target - cost(knot[1]) + w[2] - 1) / w[2];
    return (uint32_t)std::min<uint64_t>(m, samples);
}

extern "C" uint32_t ptmi_sample_split_point(int g, int n, uint32_t samples) {
    if (n <= 0 || g < 0) return 0;
    if (g >= n) return samples;
    return split_point(g, n, samples);
}

extern "C" int ptmi_trace_multi_timed(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                                      const void* groups, uint32_t n_grp, const int* devices, uint32_t n_devices,
                                      int split, uint32_t samples, const void* camera, const double* seeds,
                                      uint64_t seed_stream, const ptmi_textures* textures, double* out_rgba,
                                      ptmi_multi_timing* timing, char* err, size_t err_len) {
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point a, clk::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const clk::time_point t_start = clk::now();
    if (!out_rgba || samples == 0 || !devices || n_devices == 0 || (split != 0 && split != 1) || !camera) {
        set_err(err, err_len, "ptmi_trace_multi: bad arguments");
        return PTMI_ERR_ARG;
    }
    for (uint32_t d = 0; d < n_devices; d++) {
        const int rc = check_device(devices[d], err, err_len);
        if (rc) return rc;
    }
    // The scene is converted and its traversal index built once, on the host.
    HostScene hs;
    int rc = prepare_scene(objects, n_obj, triangles, n_tri, groups, n_grp, camera, textures, hs, err, err_len);
    if (rc) return rc;
    const clk::time_point t_prep = clk::now();
    const size_t npix = (size_t)hs.cam.width * hs.cam.height;
    const size_t frame_bytes = npix * 4 * sizeof(double);
    const int root = devices[0];
    // Device-side combine: every device's partial frame is copied (xGMI peer copy) into
    // its slot of a gather buffer on the first device, which sums the slots in device
    // order (deterministic) and normalises (tracer.cl:1184-1187).
    double* gather = nullptr;
    HIP_TRY(hipSetDevice(root));
    HIP_TRY(hipMalloc((void**)&gather, frame_bytes * n_devices));
    std::vector<int> rcs(n_devices, PTMI_OK);
    std::vector<int> peer(n_devices, -1);  // per shard: 1 direct peer access, 0 staged copy, -1 root itself
    std::vector<std::string> msgs(n_devices);
    std::vector<clk::time_point> t_rendered(n_devices, t_prep);
    // Per-device resources, released after the combine and read-back (hipFree
    // synchronises; freeing inside the device threads delayed the combine).
    std::vector<ptmi_scene*> scenes(n_devices, nullptr);
    std::vector<double*> seeds_d(n_devices, nullptr), sums_d(n_devices, nullptr);
    std::vector<hipStream_t> streams(n_devices, nullptr);
    auto shard = [&](uint32_t d) {
        char e[512] = {0};
        int& drc = rcs[d];
        const int dev = devices[d];
        ptmi_scene*& s = scenes[d];
        double*& d_seeds = seeds_d[d];
        double*& d_sums = sums_d[d];
        hipStream_t& st = streams[d];
        drc = upload_scene(hs, dev, textures, &s, e, sizeof(e));
        if (!drc && dev != root) {  // direct xGMI access to the gather buffer where the link allows it
            // hipMemcpyPeerAsync works without peer access (the runtime stages the copy), so a
            // refusal is not an error: it is reported (timing->peer_direct) and its sticky error
            // state is cleared, so it cannot surface later through launch_trace's hipGetLastError.
            int can = 0;
            peer[d] = 0;
            if (hipDeviceCanAccessPeer(&can, dev, root) == hipSuccess && can) {
                const hipError_t pe = hipDeviceEnablePeerAccess(root, 0);
                if (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled) peer[d] = 1;
            }
            (void)hipGetLastError();
        }
        if (!drc && (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess ||
                     hipMalloc((void**)&d_seeds, npix * sizeof(double)) != hipSuccess ||
                     hipMalloc((void**)&d_sums, frame_bytes) != hipSuccess)) {
            drc = PTMI_ERR_HIP;
            std::snprintf(e, sizeof(e), "device %d: allocation failed", dev);
        }
        if (!drc) {
            if (seeds) {
                if (hipMemcpyAsync(d_seeds, seeds, npix * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
                    drc = PTMI_ERR_HIP;
            } else {
                drc = ptmi_fill_seeds(d_seeds, (uint32_t)npix, seed_stream, st, e, sizeof(e));
            }
        }
        if (!drc) {
            const uint32_t s0 = split == 0 ? split_point(d, n_devices, samples) : 0;
            const uint32_t s1 = split == 0 ? split_point(d + 1, n_devices, samples) : samples;
            // an empty range writes zeros (A = 0), so every slot of the gather buffer is defined
            drc = ptmi_scene_render(s, samples, s0, s1, split == 1 ? n_devices : 1, split == 1 ? d : 0, d_seeds, d_sums,
                                    0, st, e, sizeof(e));
        }
        if (!drc && hipStreamSynchronize(st) != hipSuccess) drc = PTMI_ERR_HIP;
        t_rendered[d] = clk::now();
        if (!drc && (hipMemcpyPeerAsync(gather + (size_t)d * npix * 4, root, d_sums, dev, frame_bytes, st) !=
                         hipSuccess ||
                     hipStreamSynchronize(st) != hipSuccess)) {
            drc = PTMI_ERR_HIP;
            std::snprintf(e, sizeof(e), "device %d: peer copy to device %d failed", dev, root);
        }
        msgs[d] = e;
    };
    auto release = [&]() {
        for (uint32_t d = 0; d < n_devices; d++) {
            (void)hipSetDevice(devices[d]);
            if (streams[d]) (void)hipStreamDestroy(streams[d]);
            if (seeds_d[d]) (void)hipFree(seeds_d[d]);
            if (sums_d[d]) (void)hipFree(sums_d[d]);
            if (scenes[d]) ptmi_scene_destroy(scenes[d]);
        }
        (void)hipSetDevice(root);
        (void)hipFree(gather);
    };
    std::vector<std::thread> threads;
    for (uint32_t d = 0; d < n_devices; d++) threads.emplace_back(shard, d);
    for (auto& t : threads) t.join();
    for (uint32_t d = 0; d < n_devices; d++)
        if (rcs[d]) {
            release();
            set_err(err, err_len, "device %d: %s", devices[d], msgs[d].empty() ? "render failed" : msgs[d].c_str());
            return rcs[d];
        }
    const clk::time_point t_all_rendered = *std::max_element(t_rendered.begin(), t_rendered.end());
    hipError_t he = hipSetDevice(root);
    if (he != hipSuccess) {
        release();
        set_err(err, err_len, "hipSetDevice(%d) before the combine: %s", root, hipGetErrorString(he));
        return PTMI_ERR_HIP;
    }
    double* frame = gather;  // slot 0 is overwritten in place by the ordered sum
    he = launch_combine(gather, n_devices, npix, frame, samples, nullptr);
    if (he == hipSuccess) he = hipDeviceSynchronize();
    const clk::time_point t_combined = clk::now();
    if (he == hipSuccess) he = hipMemcpy(out_rgba, frame, frame_bytes, hipMemcpyDeviceToHost);
    const clk::time_point t_end = clk::now();
    release();
    const clk::time_point t_done = clk::now();
    if (he != hipSuccess) {
        set_err(err, err_len, "combine / read-back on device %d: %s", root, hipGetErrorString(he));
        return PTMI_ERR_HIP;
    }
    if (timing) {
        timing->prepare_ms = ms_since(t_start, t_prep);
        timing->render_ms = ms_since(t_prep, t_all_rendered);
        timing->combine_ms = ms_since(t_all_rendered, t_combined);
        timing->readback_ms = ms_since(t_combined, t_end);
        timing->total_ms = ms_since(t_start, t_done);
        timing->peer_direct = (int32_t)std::count(peer.begin(), peer.end(), 1);
        timing->peer_staged = (int32_t)std::count(peer.begin(), peer.end(), 0);
    }
    return PTMI_OK;
}

extern "C" int ptmi_trace_multi(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                                const void* groups, uint32_t n_grp, const int* devices, uint32_t n_devices, int split,
                                uint32_t samples, const void* camera, const double* seeds, uint64_t seed_stream,
                                const ptmi_textures* textures, double* out_rgba, char* err, size_t err_len) {
    return ptmi_trace_multi_timed(objects, n_obj, triangles, n_tri, groups, n_grp, devices, n_devices, split, samples,
                                  camera, seeds, seed_stream, textures, out_rgba, nullptr, err, err_len);
}

#if PTMI_STATS
namespace ptmi {
int stats_read(unsigned long long* out, int reset);
}
// DIAGNOSTIC build only: traversal counters (see PTMI_STATS in ptmi_kernels.hip).
extern "C" int ptmi_stats_read(unsigned long long* out, int reset) { return ptmi::stats_read(out, reset); }
#endif

// ---- Diagnostics (include/ptmi_diag.h) -------------------------------------------------
extern "C" int ptmi_diag_timeline_setup(void* buf_dev, uint32_t cap, char* err, size_t err_len) {
    const hipError_t e = timeline_setup((unsigned long long*)buf_dev, cap);
    if (e == hipErrorNotSupported) {
        set_err(err, err_len, "not a timeline build (make -C pathtracer-ocl_amd timeline)");
        return PTMI_ERR_UNSUPPORTED;
    }
    HIP_TRY(e);
    return PTMI_OK;
}

extern "C" int ptmi_diag_capture_setup(void* req_dev, void* res_dev, uint32_t cap, char* err, size_t err_len) {
    const hipError_t e = capture_setup((WalkReq*)req_dev, (WalkRes*)res_dev, cap);
    if (e == hipErrorNotSupported) {
        set_err(err, err_len, "not a capture build (make -C pathtracer-ocl_amd capture)");
        return PTMI_ERR_UNSUPPORTED;
    }
    HIP_TRY(e);
    return PTMI_OK;
}

extern "C" int ptmi_diag_capture_count(uint32_t* n, char* err, size_t err_len) {
    const hipError_t e = capture_count(n);
    if (e == hipErrorNotSupported) {
        set_err(err, err_len, "not a capture build");
        return PTMI_ERR_UNSUPPORTED;
    }
    HIP_TRY(e);
    return PTMI_OK;
}

extern "C" int ptmi_diag_walk(ptmi_scene* s, int mode, const void* req_dev, uint32_t n, void* res_dev,
                              uint32_t* counter_dev, void* hip_stream, float* ms, char* err, size_t err_len) {
#if !PTMI_STUDY
    (void)s, (void)mode, (void)req_dev, (void)n, (void)res_dev, (void)counter_dev, (void)hip_stream, (void)ms;
    set_err(err, err_len, "the standalone walk kernels are in the study build (make -C pathtracer-ocl_amd study)");
    return PTMI_ERR_UNSUPPORTED;
#else
    if (!s || !req_dev || !res_dev || (mode != 0 && mode != 1) || (mode == 1 && !counter_dev)) {
        set_err(err, err_len, "ptmi_diag_walk: bad arguments");
        return PTMI_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t grid = 0;
    if (mode == 1) {  // persistent: the resident waves of the pool kernel
        hipDeviceProp_t p;
        HIP_TRY(hipGetDeviceProperties(&p, s->device));
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, walk_kernel_symbol(1), 64, 0));
        grid = (uint32_t)std::max(1, per_cu) * (uint32_t)p.multiProcessorCount;
        HIP_TRY(hipMemsetAsync(counter_dev, 0, sizeof(uint32_t), st));
    }
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, st));
    const hipError_t le = launch_walk(s->dev, s->flags, mode, (const WalkReq*)req_dev, n, (WalkRes*)res_dev,
                                      counter_dev, grid, st);
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (le == hipErrorInvalidValue) {
        set_err(err, err_len, "standalone walks need an affine, untextured mesh scene");
        return PTMI_ERR_UNSUPPORTED;
    }
    HIP_TRY(le);
    if (ms) *ms = t;
    return PTMI_OK;
#endif
}

extern "C" int ptmi_diag_tile_cost(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                                   const void* groups, uint32_t n_grp, const void* camera, uint8_t* out, uint32_t n_out,
                                   char* err, size_t err_len) {
    if (!out) {
        set_err(err, err_len, "out == NULL");
        return PTMI_ERR_ARG;
    }
    HostScene hs;
    const int rc = prepare_scene(objects, n_obj, triangles, n_tri, groups, n_grp, camera, nullptr, hs, err, err_len);
    if (rc) return rc;
    const uint32_t tiles = (uint32_t)(((hs.cam.width + 7) / 8) * ((hs.cam.height + 7) / 8));
    if (n_out < tiles) {
        set_err(err, err_len, "out holds %u tiles, the frame has %u", n_out, tiles);
        return PTMI_ERR_ARG;
    }
    if (hs.flags & F_GROUPS) {
        std::vector<uint8_t> c;
        mesh_tile_cost(tile_cost_input(hs), c, tiles, [](uint32_t k) { return k; });
        std::memcpy(out, c.data(), tiles);
    } else {
        std::memset(out, 0, tiles);
    }
    return PTMI_OK;
}

extern "C" int ptmi_diag_scene_tile_cost(ptmi_scene* s, uint8_t* out, uint32_t n_out, char* err, size_t err_len) {
    if (!s || !out) {
        set_err(err, err_len, "scene or out == NULL");
        return PTMI_ERR_ARG;
    }
    const uint32_t tiles = ((s->width + 7) / 8) * ((s->height + 7) / 8);
    if (n_out < tiles) {
        set_err(err, err_len, "out holds %u tiles, the frame has %u", n_out, tiles);
        return PTMI_ERR_ARG;
    }
    if (s->flags & F_GROUPS) {  // through the scene's own cache: the classes its next ordered render sorts by
        mesh_tile_cost(s->tc_in, s->tile_cost, tiles, [](uint32_t k) { return k; });
        std::memcpy(out, s->tile_cost.data(), tiles);
    } else {
        std::memset(out, 0, tiles);
    }
    return PTMI_OK;
}

// The tiles' candidate masks of a resident scene, read back from behind its camera terms.
extern "C" int ptmi_diag_tile_cull(ptmi_scene* s, uint32_t* out, size_t n_tiles) {
    if (!s || !out) return PTMI_ERR_ARG;
    const size_t tiles = cam_tiles((int32_t)s->width, (int32_t)s->height);
    if (n_tiles < tiles) return PTMI_ERR_ARG;
    if (hipSetDevice(s->device) != hipSuccess) return PTMI_ERR_HIP;
    const uint32_t* src = cull_masks(s->dev.camg, s->dev.n_planes, s->dev.n_spheres_st);
    return hipMemcpy(out, src, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess ? PTMI_OK : PTMI_ERR_HIP;
}

// The same masks from the classifier's host build (no device call): the records prepare_scene makes,
// the camera terms by find_closest_prims' expressions (its recording form, CAM 2) in host doubles.
extern "C" int ptmi_diag_tile_cull_host(const void* objects, uint32_t n_obj, const void* triangles, uint32_t n_tri,
                                        const void* groups, uint32_t n_grp, const void* camera, uint32_t* out,
                                        size_t n_tiles, char* err, size_t err_len) {
    if (!out) {
        set_err(err, err_len, "out == NULL");
        return PTMI_ERR_ARG;
    }
    HostScene hs;
    const int rc = prepare_scene(objects, n_obj, triangles, n_tri, groups, n_grp, camera, nullptr, hs, err, err_len);
    if (rc) return rc;
    const size_t tiles = cam_tiles(hs.cam.width, hs.cam.height);
    if (n_tiles < tiles) {
        set_err(err, err_len, "out holds %zu tiles, the frame has %zu", n_tiles, tiles);
        return PTMI_ERR_ARG;
    }
    const double* co = hs.cam.origin;
    const int np = (int)hs.planes.size(), nq = (int)hs.spheres.size(), npy2 = hs.n_planes_y & ~1;
    std::vector<double> cpl((size_t)np), csp((size_t)kCamSphere * nq);
    for (int p = 0; p < np; p++) {
        const double* m = hs.planes[p].row1;
        cpl[p] = p < npy2 ? m[1] * co[1] + m[3] : ((m[0] * co[0] + m[1] * co[1]) + m[2] * co[2]) + m[3];
    }
    for (int q = 0; q < nq; q++) {
        const SphereRec& Q = hs.spheres[q];
        double* t = &csp[(size_t)kCamSphere * q];
        t[0] = Q.m0 * co[0] + Q.m3;
        t[1] = Q.m5 * co[1] + Q.m7;
        t[2] = Q.m10 * co[2] + Q.m11;
        t[3] = std::fma(t[2], t[2], std::fma(t[1], t[1], t[0] * t[0])) - 1.0;
    }
    const int tiles_x = (hs.cam.width + 7) / 8;
    for (size_t t = 0; t < tiles; t++)
        out[t] = cull_tile_mask(hs.cam, hs.planes.data(), np, hs.spheres.data(), nq, cpl.data(), csp.data(),
                                (int)(t % (size_t)tiles_x), (int)(t / (size_t)tiles_x));
    return PTMI_OK;
}

extern "C" int ptmi_diag_set_split(ptmi_scene* s, int enable) {
    if (!s) return PTMI_ERR_ARG;
#if PTMI_STUDY
    s->split = enable != 0;
    return PTMI_OK;
#else
    return enable ? PTMI_ERR_UNSUPPORTED : PTMI_OK;  // the one-kernel form is the only one here
#endif
}

extern "C" int ptmi_diag_split_passes(const ptmi_scene* s) {
#if PTMI_STUDY
    return s ? (int)s->split_passes : -1;
#else
    return s ? 0 : -1;
#endif
}

extern "C" int ptmi_diag_set_knob(ptmi_scene* s, int knob, int value) {
    if (!s) return PTMI_ERR_ARG;
    const uint32_t pos = (uint32_t)std::max(1, value);
    switch (knob) {
    case PTMI_KNOB_TAIL_TILES: s->knobs.tail_tiles = (uint32_t)std::max(0, value); return PTMI_OK;
    case PTMI_KNOB_TAIL_ITEMS: s->knobs.tail_items = pos; return PTMI_OK;
    case PTMI_KNOB_MESH_ITEMS: s->knobs.mesh_items = pos; return PTMI_OK;
    case PTMI_KNOB_MESH_ITEMS_SHARE: s->knobs.mesh_items_share = pos; return PTMI_OK;
    case PTMI_KNOB_MIN_CHUNK: s->knobs.min_chunk = pos; return PTMI_OK;
    case PTMI_KNOB_TAIL_SPLIT: s->knobs.tail_split = pos; return PTMI_OK;
    case PTMI_KNOB_TAIL_MIN: s->knobs.tail_min = (uint32_t)std::max(0, value); return PTMI_OK;
    case PTMI_KNOB_WALK_BATCH: s->dev.walk_batch = (int32_t)std::min<uint32_t>(pos, 64); return PTMI_OK;
    case PTMI_KNOB_HEMI_MESH: s->dev.hemi_mesh = value != 0; return PTMI_OK;
    case PTMI_KNOB_TILE_ORDER:
        // 2 (the order measured by the last launch) needs the item timing that only the study
        // build compiles in (ptmi_kernels.hip PTMI_TILE_COST).
        if (value < 0 || value > (PTMI_STUDY ? 2 : 1)) return PTMI_ERR_UNSUPPORTED;
        s->tile_order = value;
        s->drop_dispatch_order();
        return PTMI_OK;
#if PTMI_STUDY
    case PTMI_KNOB_SPLIT_CHUNK: s->split_chunk = pos; return PTMI_OK;
    case PTMI_KNOB_SPLIT_SLOTS: s->split_per_lane = pos; return PTMI_OK;
    case PTMI_KNOB_SPLIT_SYNC: s->split_sync = pos; return PTMI_OK;
    case PTMI_KNOB_SPLIT_BUDGET: s->split_budget = pos; return PTMI_OK;
#endif
    default: return PTMI_ERR_UNSUPPORTED;
    }
}

extern "C" int ptmi_diag_force_flags(int flags) {
    if (flags > F_GENERIC) return PTMI_ERR_ARG;
    g_force_flags.store(flags < 0 ? -1 : flags);
    return PTMI_OK;
}

extern "C" int ptmi_diag_hemi_mismatch(const ptmi_scene* s) { return s ? s->hemi_mismatch : -1; }

extern "C" int ptmi_diag_scene_flags(const ptmi_scene* s) {
    return s ? trace_kernel_flags(s->launch_flags()) : -1;
}

extern "C" int ptmi_diag_tile_ownership(const ptmi_scene* s, uint32_t tile_stride) {
    if (!s || tile_stride == 0) return -1;
    return TileOwnership::diagonal(s->launch_flags(), s->width, tile_stride, s->plan_split_chunk() != 0) ? 1 : 0;
}

// The work plan of a request (ptmi_plan.h plan_work), with no scene and no device call.
extern "C" int ptmi_diag_work_plan_host(const uint32_t* request, uint32_t n_request, uint64_t* plan_out,
                                        uint32_t n_plan, uint32_t* tiles_out, uint32_t n_tiles, char* err,
                                        size_t err_len) {
    const uint32_t* q = request;
    if (!q || !plan_out || n_request != PTMI_PLAN_REQUEST_WORDS || n_plan != PTMI_PLAN_WORDS ||
        (n_tiles && !tiles_out) || q[0] == 0 || q[1] == 0 || (uint64_t)q[0] * q[1] > (uint64_t)1 << 30 ||
        q[11] > (uint32_t)INT32_MAX) {
        set_err(err, err_len, "ptmi_diag_work_plan_host: NULL pointer, %u request / %u plan words (%d / %d), or a bad "
                              "frame or resident-wave count", n_request, n_plan, PTMI_PLAN_REQUEST_WORDS, PTMI_PLAN_WORDS);
        return PTMI_ERR_ARG;
    }
    PlanRequest rq;
    rq.width = q[0], rq.height = q[1];
    rq.samples = q[2], rq.sample_begin = q[3], rq.sample_end = q[4];
    rq.tile_stride = q[5], rq.tile_offset = q[6];
    rq.chunks = q[7];
    rq.has_list = q[8] != 0, rq.n_list = q[9];
    rq.flags = (int)q[10];
    rq.resident_waves = (int)q[11];
    rq.moments = q[12] != 0;
    rq.split_chunk = q[13];
    PlanKnobs kn;
    kn.tail_tiles = q[14], kn.tail_items = q[15], kn.mesh_items = q[16], kn.mesh_items_share = q[17];
    kn.min_chunk = q[18], kn.tail_split = q[19], kn.tail_min = q[20];
    PlanResult r;
    if (const int rc = plan_work(rq, kn, r, err, err_len)) return rc;
    const WorkPlan& wp = r.wp;
    const uint64_t out[PTMI_PLAN_WORDS] = {wp.n_whole, wp.n_tail, wp.nchunks, wp.chunk_len, wp.n_long, wp.tail_len,
                                           wp.s_begin, wp.s_end, wp.tile_stride, wp.tile_offset, r.owned_tiles,
                                           (uint64_t)r.kflags, r.own.tlist, r.pooled, r.split, r.partial_bytes};
    std::copy(out, out + PTMI_PLAN_WORDS, plan_out);
    if (!rq.has_list)  // (a caller's list is the caller's)
        for (uint32_t k = 0; k < n_tiles && k < r.owned_tiles; k++) tiles_out[k] = r.own(k);
    return PTMI_OK;
}
