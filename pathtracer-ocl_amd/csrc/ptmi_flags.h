// ptmi_flags.h -- the kernel flags of a scene and the pure predicates over them, seen by the kernels
// (ptmi_kernels.hip) and by the host (ptmi_api.cpp, ptmi_plan.h) alike.  No HIP in it.
#pragma once

namespace ptmi {

// Scene-feature flags: the host inspects the records once and launches the
// instantiation that compiles out absent object types / materials / DoF.  Every
// type or material present in the scene keeps its flag, so the result is the
// same as the generic path.
enum : int {
    F_GROUPS = 1,     // a type-4 object with BVH roots
    F_CYLCUBE = 2,    // cylinders or cubes present
    F_MATERIALS = 4,  // reflectivity != 0 or refractive index != 1 somewhere
    F_DOF = 8,        // camera aperture != 0
    F_ALL = 15,
    F_PROJ = 16,      // not affine (see dotv): the literal double4 arithmetic, generic path only
    F_TEX = 32,       // textured objects: with F_ALL | F_PROJ, the one textured instantiation
    F_TLIST = 128,    // tile-split launch with an owned-tile list (WorkPlan::tiles): affine mesh kernels only
    F_XRNG = 64,      // opt-in statistical mode (ptmi_scene_set_rng): xoshiro128** instead of noise3D,
                      // affine instantiations only; never the parity path
    F_MOM = 512,      // moment variant (ptmi_scene_render_moments): each finished path also adds
                      // (r*r + g*g) + b*b of its accumColor into the pixel's second moment (mom_add)
    F_WIDE = 256,     // affine mesh scene whose child codes need 31 bits (>= 2^15 Node4s or triangles):
                      // the affine kernel with a 32-bit LDS traversal stack (one F_ALL | F_WIDE
                      // instantiation, +- F_XRNG; ADVICE r5: such scenes had been sent to F_PROJ)
    F_GENERIC = F_ALL | F_PROJ | F_TEX  // the textured instantiation; also every bit ptmi_diag_force_flags may force
};

// Whether a launch with these scene flags can take an owned-tile list (ptmi_plan.h plan_work): the affine
// narrow-code mesh scenes in parity mode.  The study build's split form exists for the same scenes.
constexpr bool tile_list_supported(int flags) {
    return (flags & F_GROUPS) && !(flags & (F_PROJ | F_TEX | F_XRNG | F_WIDE));
}

// Whether the scene's mesh kernel is the path-pool one (ptmi_kernels.hip kPoolOf, trace_groups_pool) in the
// product build.  The host's answer ignores a library built with PTMI_POOL=0 (the study, stats, timers and
// capture libraries): their plans keep the pooled tail_min of 8, as they always have.
constexpr bool pool_kernel(int flags) { return (flags & F_GROUPS) && !(flags & (F_PROJ | F_TEX | F_XRNG)); }

// A scene's flags as its launches see them: F_XRNG added in the statistical RNG mode (ptmi_scene_set_rng).
constexpr int with_rng(int scene_flags, bool xoshiro) { return scene_flags | (xoshiro ? F_XRNG : 0); }

// The trace_kernel instantiation a launch's flags take: textured and non-affine scenes take the
// generic ones; F_XRNG exists for the affine instantiations (ptmi_scene_set_rng).
constexpr int trace_instance_flags(int flags) {
    const int mom = flags & F_MOM;  // every instantiation has its moment variant
    if (flags & F_TEX) return F_ALL | F_PROJ | F_TEX | mom;
    if (flags & F_PROJ) return F_ALL | F_PROJ | mom;
    if (flags & F_WIDE) return F_ALL | F_WIDE | (flags & F_XRNG) | mom;
    if ((flags & F_TLIST) && (flags & F_GROUPS) && !(flags & F_XRNG)) return (flags & (F_ALL | F_TLIST)) | mom;
    return (flags & (F_ALL | F_XRNG)) | mom;
}

// Every trace_kernel<FL> the library holds, written once: K(f) stands for the instantiations f and
// f | F_MOM.  ptmi_kernels.hip expands it into the kernel's symbol table and its launch switch.
#define PTMI_TRACE_INSTANCES(K)                                                                           \
    K(0) K(1) K(2) K(3) K(4) K(5) K(6) K(7) K(8) K(9) K(10) K(11) K(12) K(13) K(14) K(15)                 \
    K(F_ALL | F_PROJ) K(F_ALL | F_PROJ | F_TEX)                                                           \
    K(64) K(65) K(66) K(67) K(68) K(69) K(70) K(71) K(72) K(73) K(74) K(75) K(76) K(77) K(78) K(79)       \
    K(129) K(131) K(133) K(135) K(137) K(139) K(141) K(143)                                               \
    K(F_ALL | F_WIDE) K(F_ALL | F_WIDE | F_XRNG)

constexpr bool trace_instance_listed(int fl) {
#define PTMI_K(f) \
    if (fl == (f) || fl == ((f) | F_MOM)) return true;
    PTMI_TRACE_INSTANCES(PTMI_K)
#undef PTMI_K
    return false;
}

// Whatever flags the host hands over (every combination of the ten bits) map to a kernel that exists:
// an edit of the mapping or of the list that breaks this does not compile.
constexpr bool trace_instances_cover_all_flags() {
    for (int f = 0; f < 1024; f++)
        if (!trace_instance_listed(trace_instance_flags(f))) return false;
    return true;
}
static_assert(trace_instances_cover_all_flags(), "trace_instance_flags() names an instantiation PTMI_TRACE_INSTANCES lacks");

}  // namespace ptmi
