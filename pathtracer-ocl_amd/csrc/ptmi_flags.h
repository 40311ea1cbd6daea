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

}  // namespace ptmi
