"""ctypes binding of libptmi.so (include/ptmi.h).

``Trace`` mirrors the reference's Go entry point
``internal/ocl.Trace(objects, triangles, groups, deviceIndex, samples, camera,
textures, sphereTextures, cubeTextures) []float64`` (ocltracer.go:98-226): same
argument meaning, same record bytes, same float64 RGBA result.  Where the Go code
calls ``logrus.Fatalf`` this raises ``PtmiError`` (the library returned an error
code; nothing falls back to another implementation).

``Scene`` exposes the resident-scene API (scene uploaded to HBM once, frames
rendered from device buffers on a caller's HIP stream) used by bench.py and
the multi-GPU driver; device buffers are passed as raw pointers (e.g.
``tensor.data_ptr()``), so the C ABI stays free of torch types.
"""
import ctypes
import os

import numpy as np

from . import _runtime, layout
from .textures import TextureSet

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTMI_LIB", os.path.join(_HERE, "..", "build", "libptmi.so"))
# DIAGNOSTIC study library (make -C pathtracer-ocl_amd study): the product plus the split
# execution form, the standalone walk kernels and the measured tile order.
STUDY_LIB_PATH = os.path.join(_HERE, "..", "build", "libptmi_study.so")

PTMI_OK, PTMI_ERR_ARG, PTMI_ERR_DEVICE, PTMI_ERR_HIP, PTMI_ERR_UNSUPPORTED, PTMI_ERR_NOMEM = 0, -1, -2, -3, -4, -5
RNG_NOISE3D, RNG_XOSHIRO = 0, 1  # ptmi_scene_set_rng: parity (default) / opt-in statistical mode
# ptmi_diag_set_knob (include/ptmi_diag.h): work-plan knobs of a resident scene
(KNOB_TAIL_TILES, KNOB_TAIL_ITEMS, KNOB_MESH_ITEMS, KNOB_MIN_CHUNK, KNOB_TILE_ORDER, KNOB_SPLIT_CHUNK,
 KNOB_SPLIT_SLOTS, KNOB_SPLIT_SYNC, KNOB_SPLIT_BUDGET, KNOB_TAIL_SPLIT, KNOB_MESH_ITEMS_SHARE, KNOB_TAIL_MIN,
 KNOB_WALK_BATCH, KNOB_HEMI_MESH) = range(1, 15)

EXPORTS = ("ptmi_trace", "ptmi_device_count", "ptmi_device_name", "ptmi_scene_create", "ptmi_scene_destroy",
           "ptmi_scene_size", "ptmi_scene_render", "ptmi_finalize", "ptmi_fill_seeds", "ptmi_build_info",
           "ptmi_scene_set_timing", "ptmi_scene_kernel_time", "ptmi_trace_multi", "ptmi_scene_create_textured",
           "ptmi_trace_multi_timed", "ptmi_sample_split_point", "ptmi_combine_frames",
           "ptmi_scene_set_rng", "ptmi_index_stats", "ptmi_scene_render_moments", "ptmi_error_map", "ptmi_accumulate",
           "ptmi_scene_render_tiles", "ptmi_select_tiles", "ptmi_finalize_counts", "ptmi_scene_features",
           "ptmi_denoise", "ptmi_denoise_work_bytes", "ptmi_scene_set_camera", "ptmi_reproject",
           "ptmi_scene_set_objects", "ptmi_motion_table", "ptmi_reproject_motion", "ptmi_history_gather",
           "ptmi_rectify", "ptmi_scene_features_chain", "ptmi_variance_estimate")
FEATURE_DOUBLES = 12    # PTMI_FEATURE_DOUBLES: doubles per pixel of Scene.features
HISTORY_DOUBLES = 8     # PTMI_HISTORY_DOUBLES: doubles per pixel of a reproject history
MOTION_DOUBLES = 24     # PTMI_MOTION_DOUBLES: doubles per object of a motion table
MOMENT_DOUBLES = 8      # PTMI_MOMENT_DOUBLES: doubles per pixel of a variance_estimate moment record
DENOISE_DEMODULATE = 1  # PTMI_DENOISE_DEMODULATE


class MultiTiming(ctypes.Structure):
    """ptmi_multi_timing (include/ptmi.h): wall-clock phases of ptmi_trace_multi, ms."""
    _fields_ = [(n, ctypes.c_double) for n in ("prepare_ms", "render_ms", "combine_ms", "readback_ms", "total_ms")] + \
        [("peer_direct", ctypes.c_int32), ("peer_staged", ctypes.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DenoiseParams(ctypes.Structure):
    """ptmi_denoise_params (include/ptmi.h); the constructor's defaults are the library's."""
    _fields_ = [("iterations", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("sigma_l", ctypes.c_double),
                ("sigma_d", ctypes.c_double), ("normal_power", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def __init__(self, iterations=5, flags=DENOISE_DEMODULATE, sigma_l=4.0, sigma_d=0.01, normal_power=7):
        super().__init__(iterations, flags, sigma_l, sigma_d, normal_power, 0)


class ReprojectParams(ctypes.Structure):
    """ptmi_reproject_params (include/ptmi.h); the constructor's defaults are the library's."""
    _fields_ = [("max_history", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("normal_cos", ctypes.c_double),
                ("plane_dist", ctypes.c_double), ("min_weight", ctypes.c_double)]

    def __init__(self, max_history=32, flags=0, normal_cos=0.9, plane_dist=0.02, min_weight=0.05):
        super().__init__(max_history, flags, normal_cos, plane_dist, min_weight)


class RectifyParams(ctypes.Structure):
    """ptmi_rectify_params (include/ptmi.h); the constructor's defaults are the library's."""
    _fields_ = [("radius", ctypes.c_uint32), ("min_count", ctypes.c_uint32), ("gamma", ctypes.c_double),
                ("max_history", ctypes.c_uint32), ("flags", ctypes.c_uint32)]

    def __init__(self, radius=3, min_count=9, gamma=3.0, max_history=32, flags=0):
        super().__init__(radius, min_count, gamma, max_history, flags)


class VarianceParams(ctypes.Structure):
    """ptmi_variance_params (include/ptmi.h); the constructor's defaults are the library's."""
    _fields_ = [("max_history", ctypes.c_uint32), ("min_temporal", ctypes.c_uint32), ("radius", ctypes.c_uint32),
                ("min_count", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("normal_cos", ctypes.c_double),
                ("plane_dist", ctypes.c_double), ("min_weight", ctypes.c_double), ("window_normal_cos", ctypes.c_double)]

    def __init__(self, max_history=32, min_temporal=4, radius=3, min_count=9, flags=0, normal_cos=0.9, plane_dist=0.02,
                 min_weight=0.05, window_normal_cos=0.9):
        super().__init__(max_history, min_temporal, radius, min_count, flags, normal_cos, plane_dist, min_weight,
                         window_normal_cos)


class PtmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libptmi error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load_library(path=None):
    """Load libptmi.so (raises if it is missing: there is no fallback path)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = os.path.abspath(path or LIB_PATH)
    _runtime.preload()
    if not os.path.exists(p):
        raise FileNotFoundError("libptmi.so not built (%s): run `make -C pathtracer-ocl_amd`" % p)
    lib = ctypes.CDLL(p)
    vp, u32, i32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    cp = ctypes.c_char_p
    lib.ptmi_trace.restype = i32
    lib.ptmi_trace.argtypes = [vp, u32, vp, u32, vp, u32, i32, u32, vp, vp, ctypes.c_uint64, vp, vp, cp, sz]
    lib.ptmi_trace_multi.restype = i32
    lib.ptmi_trace_multi.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, i32, u32, vp, vp, ctypes.c_uint64, vp, vp,
                                     cp, sz]
    lib.ptmi_trace_multi_timed.restype = i32
    lib.ptmi_trace_multi_timed.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, i32, u32, vp, vp, ctypes.c_uint64, vp,
                                           vp, ctypes.POINTER(MultiTiming), cp, sz]
    if hasattr(lib, "ptmi_combine_frames"):
        lib.ptmi_combine_frames.restype = i32
        lib.ptmi_combine_frames.argtypes = [vp, u32, u32, vp, u32, vp, cp, sz]
    lib.ptmi_sample_split_point.restype = u32
    lib.ptmi_sample_split_point.argtypes = [i32, i32, u32]
    lib.ptmi_device_count.restype = i32
    lib.ptmi_device_count.argtypes = []
    lib.ptmi_device_name.restype = i32
    lib.ptmi_device_name.argtypes = [i32, cp, sz]
    lib.ptmi_scene_create.restype = i32
    lib.ptmi_scene_create.argtypes = [i32, vp, u32, vp, u32, vp, u32, vp, ctypes.POINTER(vp), cp, sz]
    lib.ptmi_scene_create_textured.restype = i32
    lib.ptmi_scene_create_textured.argtypes = [i32, vp, u32, vp, u32, vp, u32, vp, vp, ctypes.POINTER(vp), cp, sz]
    lib.ptmi_scene_destroy.restype = None
    lib.ptmi_scene_destroy.argtypes = [vp]
    lib.ptmi_scene_size.restype = i32
    lib.ptmi_scene_size.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.ptmi_scene_render.restype = i32
    lib.ptmi_scene_render.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp, u32, vp, cp, sz]
    if hasattr(lib, "ptmi_scene_render_moments"):  # (diagnostic libraries of earlier rounds lack them)
        lib.ptmi_scene_render_moments.restype = i32
        lib.ptmi_scene_render_moments.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp, vp, u32, vp, cp, sz]
        lib.ptmi_error_map.restype = i32
        lib.ptmi_error_map.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, cp, sz]
        lib.ptmi_accumulate.restype = i32
        lib.ptmi_accumulate.argtypes = [vp, vp, sz, vp, cp, sz]
    if hasattr(lib, "ptmi_scene_render_tiles"):  # (likewise)
        lib.ptmi_scene_render_tiles.restype = i32
        lib.ptmi_scene_render_tiles.argtypes = [vp, u32, u32, u32, vp, u32, vp, vp, vp, u32, vp, cp, sz]
        lib.ptmi_select_tiles.restype = i32
        lib.ptmi_select_tiles.argtypes = [vp, vp, u32, ctypes.c_double, vp, vp, vp, cp, sz]
        lib.ptmi_finalize_counts.restype = i32
        lib.ptmi_finalize_counts.argtypes = [vp, vp, u32, vp, cp, sz]
    if hasattr(lib, "ptmi_denoise"):  # (likewise)
        lib.ptmi_scene_features.restype = i32
        lib.ptmi_scene_features.argtypes = [vp, vp, vp, cp, sz]
        lib.ptmi_denoise_work_bytes.restype = sz
        lib.ptmi_denoise_work_bytes.argtypes = [u32, u32]
        lib.ptmi_denoise.restype = i32
        lib.ptmi_denoise.argtypes = [vp, vp, vp, u32, u32, ctypes.POINTER(DenoiseParams), vp, vp, vp, sz, vp, cp, sz]
    if hasattr(lib, "ptmi_scene_features_chain"):  # (likewise)
        lib.ptmi_scene_features_chain.restype = i32
        lib.ptmi_scene_features_chain.argtypes = [vp, vp, u32, ctypes.c_double, vp, cp, sz]
    if hasattr(lib, "ptmi_reproject"):  # (likewise)
        lib.ptmi_scene_set_camera.restype = i32
        lib.ptmi_scene_set_camera.argtypes = [vp, vp, cp, sz]
        lib.ptmi_reproject.restype = i32
        lib.ptmi_reproject.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, ctypes.POINTER(ReprojectParams), vp, vp, vp,
                                       vp, cp, sz]
    if hasattr(lib, "ptmi_reproject_motion"):  # (likewise)
        lib.ptmi_scene_set_objects.restype = i32
        lib.ptmi_scene_set_objects.argtypes = [vp, vp, u32, cp, sz]
        lib.ptmi_motion_table.restype = i32
        lib.ptmi_motion_table.argtypes = [vp, vp, u32, vp, vp, cp, sz]
        lib.ptmi_reproject_motion.restype = i32
        lib.ptmi_reproject_motion.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, ctypes.POINTER(ReprojectParams), vp, vp,
                                              vp, vp, u32, vp, cp, sz]
    if hasattr(lib, "ptmi_rectify"):  # (likewise)
        lib.ptmi_history_gather.restype = i32
        lib.ptmi_history_gather.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, ctypes.POINTER(ReprojectParams), vp, vp,
                                            u32, vp, cp, sz]
        lib.ptmi_rectify.restype = i32
        lib.ptmi_rectify.argtypes = [vp, vp, vp, vp, u32, u32, ctypes.POINTER(RectifyParams), vp, vp, vp, vp, cp, sz]
    if hasattr(lib, "ptmi_variance_estimate"):  # (likewise)
        lib.ptmi_variance_estimate.restype = i32
        lib.ptmi_variance_estimate.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, ctypes.POINTER(VarianceParams), vp, vp,
                                               vp, u32, vp, cp, sz]
    if hasattr(lib, "ptmi_diag_scene_tile_cost"):
        lib.ptmi_diag_scene_tile_cost.restype = i32
        lib.ptmi_diag_scene_tile_cost.argtypes = [vp, vp, u32, cp, sz]
    if hasattr(lib, "ptmi_diag_tile_cull"):
        lib.ptmi_diag_tile_cull.restype = i32
        lib.ptmi_diag_tile_cull.argtypes = [vp, vp, sz]
        lib.ptmi_diag_tile_cull_host.restype = i32
        lib.ptmi_diag_tile_cull_host.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp, sz, cp, sz]
    if hasattr(lib, "ptmi_diag_work_plan_host"):
        lib.ptmi_diag_work_plan_host.restype = i32
        lib.ptmi_diag_work_plan_host.argtypes = [vp, u32, vp, u32, vp, u32, cp, sz]
    lib.ptmi_finalize.restype = i32
    lib.ptmi_finalize.argtypes = [vp, vp, u32, u32, vp, cp, sz]
    lib.ptmi_fill_seeds.restype = i32
    lib.ptmi_fill_seeds.argtypes = [vp, u32, ctypes.c_uint64, vp, cp, sz]
    if hasattr(lib, "ptmi_scene_set_rng"):  # (older diagnostic builds lack it; tests/test_abi.py checks the product)
        lib.ptmi_scene_set_rng.restype = i32
        lib.ptmi_scene_set_rng.argtypes = [vp, i32, cp, sz]
    lib.ptmi_scene_set_timing.restype = i32
    lib.ptmi_scene_set_timing.argtypes = [vp, i32]
    lib.ptmi_scene_kernel_time.restype = i32
    lib.ptmi_scene_kernel_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32), cp, sz]
    lib.ptmi_build_info.restype = cp
    lib.ptmi_build_info.argtypes = []
    if hasattr(lib, "ptmi_index_stats"):
        lib.ptmi_index_stats.restype = i32
        lib.ptmi_index_stats.argtypes = [vp, u32, vp, u32, vp, u32, vp, ctypes.POINTER(ctypes.c_double), i32, cp, sz]
    for name, args in (("ptmi_diag_set_knob", [vp, i32, i32]), ("ptmi_diag_force_flags", [i32]),
                       ("ptmi_diag_hemi_mismatch", [vp]), ("ptmi_diag_set_split", [vp, i32]),
                       ("ptmi_diag_split_passes", [vp]), ("ptmi_diag_scene_flags", [vp]),
                       ("ptmi_diag_tile_ownership", [vp, u32]), ("ptmi_diag_denoise_variant", [i32])):
        if hasattr(lib, name):  # (diagnostic libraries of earlier rounds lack some)
            getattr(lib, name).restype = i32
            getattr(lib, name).argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(rc, err):
    if rc != PTMI_OK:
        raise PtmiError(rc, err.value.decode(errors="replace"))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and len(a) else None


def _vp(address):
    """A device address (or a stream) as the library takes it; 0 and None are NULL."""
    return ctypes.c_void_p(address or None)


def _params(cls, params):
    """A parameter record of class `cls` from None (the library's defaults), a `cls` or a dict of some fields."""
    if params is None or isinstance(params, cls):
        return params
    return cls(**dict(params))


def _ref(p):
    return ctypes.byref(p) if p is not None else None


def _records(objects, triangles, groups, camera):
    objects = np.ascontiguousarray(objects)
    triangles = np.ascontiguousarray(triangles) if triangles is not None else np.zeros(0, layout.TRIANGLE_DTYPE)
    groups = np.ascontiguousarray(groups) if groups is not None else np.zeros(0, layout.GROUP_DTYPE)
    camera = np.ascontiguousarray(np.asarray(camera).reshape(1))
    for arr, dt, name in ((objects, layout.OBJECT_DTYPE, "objects"), (triangles, layout.TRIANGLE_DTYPE, "triangles"),
                          (groups, layout.GROUP_DTYPE, "groups"), (camera, layout.CAMERA_DTYPE, "camera")):
        if arr.dtype.itemsize != dt.itemsize:
            raise TypeError("%s: expected %d-byte records, got %d" % (name, dt.itemsize, arr.dtype.itemsize))
    return objects, triangles, groups, camera


def device_count():
    return load_library().ptmi_device_count()


def device_name(i):
    buf = ctypes.create_string_buffer(256)
    rc = load_library().ptmi_device_name(i, buf, len(buf))
    if rc:
        raise PtmiError(rc, "no device %d" % i)
    return buf.value.decode()


def Trace(objects, triangles, groups, deviceIndex, samples, camera, textures=None, sphereTextures=None,
          cubeTextures=None, seeds=None, seed_stream=0):
    """Drop-in for ocl.Trace (ocltracer.go:98-100).  Returns float64 RGBA, len W*H*4.

    ``seeds``: W*H per-pixel seeds (the Go side's rand.Float64() per pixel); None
    lets the library generate them from ``seed_stream``.  ``textures`` /
    ``sphereTextures`` / ``cubeTextures``: lists of H x W x 4 uint8 NRGBA images
    (ptmi/textures.py), or None.
    """
    tex = TextureSet(textures, sphereTextures, cubeTextures)
    lib = load_library()
    objects, triangles, groups, camera = _records(objects, triangles, groups, camera)
    w, h = int(camera["width"][0]), int(camera["height"][0])
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.float64)
        if seeds.size != w * h:
            raise ValueError("seeds: expected %d values, got %d" % (w * h, seeds.size))
    out = np.empty(w * h * 4, dtype=np.float64)
    err = ctypes.create_string_buffer(1024)
    rc = lib.ptmi_trace(_ptr(objects), len(objects), _ptr(triangles), len(triangles), _ptr(groups), len(groups),
                        int(deviceIndex), int(samples), _ptr(camera), _ptr(seeds), int(seed_stream), tex.pointer(),
                        out.ctypes.data_as(ctypes.c_void_p), err, len(err))
    _check(rc, err)
    return out


def TraceMulti(objects, triangles, groups, devices, split, samples, camera, textures=None, sphereTextures=None,
               cubeTextures=None, seeds=None, seed_stream=0):
    """ptmi_trace_multi_timed: the frame over `devices` (an index may repeat) with a
    sample (split="sample") or 8x8-tile (split="tile") split, combined on device.
    Returns (float64 RGBA of len W*H*4, {phase: ms})."""
    tex = TextureSet(textures, sphereTextures, cubeTextures)
    lib = load_library()
    objects, triangles, groups, camera = _records(objects, triangles, groups, camera)
    w, h = int(camera["width"][0]), int(camera["height"][0])
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.float64)
        if seeds.size != w * h:
            raise ValueError("seeds: expected %d values, got %d" % (w * h, seeds.size))
    if split not in ("sample", "tile"):
        raise ValueError("split must be 'sample' or 'tile'")
    devs = (ctypes.c_int * len(devices))(*devices)
    out = np.empty(w * h * 4, dtype=np.float64)
    timing = MultiTiming()
    err = ctypes.create_string_buffer(1024)
    rc = lib.ptmi_trace_multi_timed(_ptr(objects), len(objects), _ptr(triangles), len(triangles), _ptr(groups),
                                    len(groups), devs, len(devices), 0 if split == "sample" else 1, int(samples),
                                    _ptr(camera), _ptr(seeds), int(seed_stream), tex.pointer(),
                                    out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(timing), err, len(err))
    _check(rc, err)
    return out, timing.as_dict()


def combine_frames(parts_ptr, n_parts, n_pixels, out_ptr, samples, stream=0):
    """ptmi_combine_frames: n_parts partial frames (device memory, back to back) summed
    in part order and normalised into out_ptr (may equal parts_ptr)."""
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_combine_frames(_vp(parts_ptr), int(n_parts), int(n_pixels),
                                              _vp(out_ptr), int(samples), _vp(stream),
                                              err, len(err)), err)


def index_stats(objects, triangles, groups, camera):
    """ptmi_index_stats (host only): summary of the traversal index the library builds
    for these records -- {nodes4, slots, box_area, inf_bounds, max_scale_exp, roots, depth}."""
    objects, triangles, groups, camera = _records(objects, triangles, groups, camera)
    out = (ctypes.c_double * 8)()
    err = ctypes.create_string_buffer(1024)
    _check(load_library().ptmi_index_stats(_ptr(objects), len(objects), _ptr(triangles), len(triangles),
                                           _ptr(groups), len(groups), _ptr(camera), out, 8, err, len(err)), err)
    return dict(zip(("nodes4", "slots", "box_area", "inf_bounds", "max_scale_exp", "roots", "depth", "leaf_bit"),
                    list(out)))


def tile_cull_host(objects, triangles, groups, camera):
    """ptmi_diag_tile_cull_host (host only): the camera-ray stage's candidate mask of every 8x8 tile,
    raster order -- bit i plane i, bit 16 + i scale+translate sphere i; all ones where nothing is culled."""
    objects, triangles, groups, camera = _records(objects, triangles, groups, camera)
    rec = camera.view(layout.CAMERA_DTYPE)
    w, h = int(rec["width"][0]), int(rec["height"][0])
    out = np.zeros(((w + 7) // 8) * ((h + 7) // 8), dtype=np.uint32)
    err = ctypes.create_string_buffer(1024)
    _check(load_library().ptmi_diag_tile_cull_host(_ptr(objects), len(objects), _ptr(triangles), len(triangles),
                                                   _ptr(groups), len(groups), _ptr(camera),
                                                   out.ctypes.data_as(ctypes.c_void_p), len(out), err, len(err)), err)
    return out


# ptmi_diag_work_plan_host: the request's words and the plan's, in the order include/ptmi_diag.h gives.
PLAN_REQUEST_FIELDS = ("width", "height", "samples", "sample_begin", "sample_end", "tile_stride", "tile_offset",
                       "chunks", "has_list", "n_list", "flags", "resident_waves", "moments", "split_chunk",
                       "tail_tiles", "tail_items", "mesh_items", "mesh_items_share", "min_chunk", "tail_split",
                       "tail_min")
PLAN_FIELDS = ("n_whole", "n_tail", "nchunks", "chunk_len", "n_long", "tail_len", "s_begin", "s_end", "tile_stride",
               "tile_offset", "owned_tiles", "launch_flags", "tlist", "pooled", "split", "partial_bytes")


def work_plan_host(request, n_tiles=0):
    """ptmi_diag_work_plan_host (host only, no scene): the work plan a render makes of `request` (a sequence of
    the PLAN_REQUEST_FIELDS values, or a dict of them).  Returns ({PLAN_FIELDS name: value}, the first
    min(n_tiles, owned_tiles) owned tiles' raster indices); raises PtmiError as the render would."""
    if isinstance(request, dict):
        request = [request[k] for k in PLAN_REQUEST_FIELDS]
    req = np.ascontiguousarray(request, dtype=np.uint32)
    plan = np.zeros(len(PLAN_FIELDS), dtype=np.uint64)
    tiles = np.zeros(int(n_tiles), dtype=np.uint32)
    err = ctypes.create_string_buffer(1024)
    _check(load_library().ptmi_diag_work_plan_host(_ptr(req), len(req), _ptr(plan), len(plan), _ptr(tiles), len(tiles),
                                                   err, len(err)), err)
    d = {k: int(v) for k, v in zip(PLAN_FIELDS, plan)}
    has_list = bool(req[PLAN_REQUEST_FIELDS.index("has_list")])  # (a caller's list is the caller's: no tiles)
    return d, tiles[:0 if has_list else min(len(tiles), d["owned_tiles"])]


class force_flags:
    """Context manager (ptmi_diag_force_flags): scenes created inside it -- by Trace or
    Scene -- launch the kernel instantiation `flags` instead of their own (test hook for
    the generic instantiations)."""

    def __init__(self, flags, lib=None):
        self.flags, self.lib = int(flags), lib or load_library()

    def __enter__(self):
        _check(self.lib.ptmi_diag_force_flags(self.flags), ctypes.create_string_buffer(b"bad flags"))
        return self

    def __exit__(self, *exc):
        self.lib.ptmi_diag_force_flags(-1)
        return False


def sample_split_point(g, n, samples):
    """The library's cost-balanced sample split (ptmi_sample_split_point)."""
    return load_library().ptmi_sample_split_point(int(g), int(n), int(samples))


class Scene:
    """A scene resident on one device (ptmi_scene_*)."""

    def __init__(self, device_index, objects, triangles, groups, camera, textures=None, sphereTextures=None,
                 cubeTextures=None, lib=None):
        # lib: another build of the library (e.g. load_library(STUDY_LIB_PATH)); default the product
        self._lib = lib or load_library()
        objects, triangles, groups, camera = _records(objects, triangles, groups, camera)
        tex = TextureSet(textures, sphereTextures, cubeTextures)
        handle = ctypes.c_void_p()
        err = ctypes.create_string_buffer(1024)
        rc = self._lib.ptmi_scene_create_textured(int(device_index), _ptr(objects), len(objects), _ptr(triangles),
                                                  len(triangles), _ptr(groups), len(groups), _ptr(camera),
                                                  tex.pointer(), ctypes.byref(handle), err, len(err))
        _check(rc, err)
        self._h = handle
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        self._lib.ptmi_scene_size(self._h, ctypes.byref(w), ctypes.byref(h))
        self.width, self.height = w.value, h.value

    def render(self, samples, sample_begin, sample_end, seeds_ptr, sums_ptr, tile_stride=1, tile_offset=0,
               chunks=0, stream=0):
        err = ctypes.create_string_buffer(1024)
        rc = self._lib.ptmi_scene_render(self._h, samples, sample_begin, sample_end, tile_stride, tile_offset,
                                         _vp(seeds_ptr), _vp(sums_ptr), chunks,
                                         _vp(stream), err, len(err))
        _check(rc, err)

    def render_moments(self, samples, sample_begin, sample_end, seeds_ptr, sums_ptr, sq_ptr, tile_stride=1,
                       tile_offset=0, chunks=0, stream=0):
        """ptmi_scene_render_moments: render(), also writing sq_ptr[W*H] -- per owned pixel the sum over
        the range's paths of (r*r + g*g) + b*b, 0 elsewhere.  The sums are render()'s bit for bit."""
        err = ctypes.create_string_buffer(1024)
        rc = self._lib.ptmi_scene_render_moments(self._h, samples, sample_begin, sample_end, tile_stride, tile_offset,
                                                 _vp(seeds_ptr), _vp(sums_ptr),
                                                 _vp(sq_ptr), chunks, _vp(stream), err,
                                                 len(err))
        _check(rc, err)

    def render_tiles(self, samples, sample_begin, sample_end, tiles_ptr, n_tiles, seeds_ptr, sums_ptr, sq_ptr,
                     chunks=0, stream=0):
        """ptmi_scene_render_tiles: render_moments() on the n_tiles 8x8 tiles whose raster indices
        (uint32, distinct) are at tiles_ptr in device memory; every other pixel of sums_ptr and sq_ptr
        is set to 0.  An index past the frame's tiles is skipped."""
        err = ctypes.create_string_buffer(1024)
        rc = self._lib.ptmi_scene_render_tiles(self._h, samples, sample_begin, sample_end,
                                               _vp(tiles_ptr), int(n_tiles),
                                               _vp(seeds_ptr), _vp(sums_ptr),
                                               _vp(sq_ptr), chunks, _vp(stream), err,
                                               len(err))
        _check(rc, err)

    def finalize_counts(self, sums_ptr, out_ptr, stream=0):
        """ptmi_finalize_counts over the scene's pixels: finalize() by each pixel's own count."""
        finalize_counts(sums_ptr, out_ptr, self.width * self.height, stream=stream)

    def finalize(self, sums_ptr, out_ptr, samples, stream=0):
        err = ctypes.create_string_buffer(1024)
        rc = self._lib.ptmi_finalize(_vp(sums_ptr), _vp(out_ptr),
                                     self.width * self.height, samples, _vp(stream), err, len(err))
        _check(rc, err)

    def features(self, feat_ptr, stream=0, chain=False, max_chain=8, reflect_min=0.5):
        """ptmi_scene_features: the first-hit records of the pinhole rays through the pixel centres,
        W*H*FEATURE_DOUBLES doubles at feat_ptr (position, t, normal, object id, albedo, 0).
        chain=True: ptmi_scene_features_chain instead -- the rays followed through at most max_chain
        mirrors (reflectivity >= reflect_min) and glass interfaces to the first surface that is neither,
        recorded at its virtual position, with the chain's length in slot [11]."""
        err = ctypes.create_string_buffer(256)
        if chain:
            _check(self._lib.ptmi_scene_features_chain(self._h, _vp(feat_ptr), int(max_chain),
                                                       float(reflect_min), _vp(stream), err, len(err)),
                   err)
            return
        _check(self._lib.ptmi_scene_features(self._h, _vp(feat_ptr), _vp(stream), err,
                                             len(err)), err)

    def set_camera(self, camera_record):
        """ptmi_scene_set_camera: a new 256-byte camera record of the scene's width and height.  The scene
        then renders bit for bit what a scene freshly created with this camera renders; only the camera
        is converted and uploaded.  Blocks until the device's earlier work and the upload are done."""
        cam = np.ascontiguousarray(np.asarray(camera_record).reshape(1))
        if cam.dtype.itemsize != layout.CAMERA_DTYPE.itemsize:
            raise TypeError("camera: expected %d-byte records, got %d" % (layout.CAMERA_DTYPE.itemsize,
                                                                          cam.dtype.itemsize))
        err = ctypes.create_string_buffer(512)
        _check(self._lib.ptmi_scene_set_camera(self._h, _ptr(cam), err, len(err)), err)

    def set_objects(self, objects):
        """ptmi_scene_set_objects: new 1024-byte object records, as many as the scene was created with and
        of the same types (a group keeps its roots and its box).  The scene then renders bit for bit
        what a scene freshly created with these objects renders; no traversal index is rebuilt.  Blocks
        until the device's earlier work and the uploads are done."""
        objs = np.ascontiguousarray(objects)
        if objs.dtype.itemsize != layout.OBJECT_DTYPE.itemsize:
            raise TypeError("objects: expected %d-byte records, got %d" % (layout.OBJECT_DTYPE.itemsize,
                                                                           objs.dtype.itemsize))
        err = ctypes.create_string_buffer(512)
        _check(self._lib.ptmi_scene_set_objects(self._h, _ptr(objs), len(objs), err, len(err)), err)

    def tile_cost(self):
        """ptmi_diag_scene_tile_cost: the static dispatch class (0..9) of every 8x8 tile as the scene's
        next ordered render sees it, raster order (all 0 without meshes)."""
        tiles = ((self.width + 7) // 8) * ((self.height + 7) // 8)
        out = np.zeros(tiles, dtype=np.uint8)
        err = ctypes.create_string_buffer(256)
        _check(self._lib.ptmi_diag_scene_tile_cost(self._h, out.ctypes.data_as(ctypes.c_void_p), tiles, err, len(err)),
               err)
        return out

    def tile_cull(self):
        """ptmi_diag_tile_cull: the scene's candidate masks (tile_cull_host's layout) as the device holds
        them for its current camera."""
        out = np.zeros(((self.width + 7) // 8) * ((self.height + 7) // 8), dtype=np.uint32)
        rc = self._lib.ptmi_diag_tile_cull(self._h, out.ctypes.data_as(ctypes.c_void_p), len(out))
        _check(rc, ctypes.create_string_buffer(b"ptmi_diag_tile_cull failed"))
        return out

    def set_rng(self, mode):
        """RNG_NOISE3D (default, the reference's noise3D bit for bit) or RNG_XOSHIRO (the
        opt-in statistical mode: images converge to the same expectation, not equal)."""
        err = ctypes.create_string_buffer(256)
        _check(self._lib.ptmi_scene_set_rng(self._h, int(mode), err, len(err)), err)

    def set_split(self, enable=True):
        """Diagnostics (include/ptmi_diag.h): mesh scenes in the split form (study library
        only) or the (default) one-kernel form.  Returns False when the library lacks it."""
        if not hasattr(self._lib, "ptmi_diag_set_split"):
            return False
        return self._lib.ptmi_diag_set_split(self._h, 1 if enable else 0) == 0

    def split_passes(self):
        return self._lib.ptmi_diag_split_passes(self._h)

    def set_knob(self, knob, value):
        """ptmi_diag_set_knob: a work-plan knob (KNOB_*); returns the library's status code
        (PTMI_ERR_UNSUPPORTED for a knob or value this build lacks)."""
        return self._lib.ptmi_diag_set_knob(self._h, int(knob), int(value))

    def hemi_mismatch(self):
        """ptmi_diag_hemi_mismatch: hemisphere-table records where the generic operator
        sequences differ from the affine ones the table holds (0 expected)."""
        return self._lib.ptmi_diag_hemi_mismatch(self._h)

    def kernel_flags(self):
        """ptmi_diag_scene_flags: F_* flags of the trace_kernel instantiation this scene launches."""
        return self._lib.ptmi_diag_scene_flags(self._h)

    def tile_ownership(self, tile_stride):
        """ptmi_diag_tile_ownership: 'diagonal' or 'raster', the tile ownership a tile-split render
        with this stride uses (the library's own decision; ptmi/dist.py tile_owner_mask takes it)."""
        r = self._lib.ptmi_diag_tile_ownership(self._h, int(tile_stride))
        if r < 0:
            raise PtmiError(PTMI_ERR_ARG, "tile_ownership: bad stride %r" % (tile_stride,))
        return "diagonal" if r == 1 else "raster"

    def set_timing(self, enable=True):
        self._lib.ptmi_scene_set_timing(self._h, 1 if enable else 0)

    def kernel_time(self):
        """(summed trace_kernel ms, launches) since the last call (waits for them)."""
        ms, n = ctypes.c_double(), ctypes.c_uint32()
        err = ctypes.create_string_buffer(512)
        _check(self._lib.ptmi_scene_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(n), err, len(err)), err)
        return ms.value, n.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ptmi_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_seeds(seeds_ptr, n, seed_stream, stream=0):
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_fill_seeds(_vp(seeds_ptr), n, seed_stream, _vp(stream), err, len(err)), err)


def error_map(sums_ptr, sq_ptr, width, height, stats_ptr, se_ptr=0, tile_err_ptr=0, stream=0):
    """ptmi_error_map: from frame sums (W*H*4: r, g, b, n) and second moments (W*H), the standard
    error of each pixel's mean into se_ptr (W*H doubles, optional), each 8x8 tile's rms standard
    error into tile_err_ptr (raster order, optional) and stats_ptr[4] = (rms standard error, largest
    finite one, mean of the pixel means, pixel count) over the pixels with n >= 2.  The formula is
    ptmi/error.py error_map_reference."""
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_error_map(_vp(sums_ptr), _vp(sq_ptr), int(width), int(height), _vp(se_ptr),
                                         _vp(tile_err_ptr), _vp(stats_ptr), _vp(stream), err, len(err)), err)


def accumulate(dst_ptr, src_ptr, n, stream=0):
    """ptmi_accumulate: dst[k] += src[k] over n doubles of device memory (batches of sums, whose
    fourth slots -- the sample counts -- add too, and of second moments)."""
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_accumulate(_vp(dst_ptr), _vp(src_ptr), int(n), _vp(stream), err, len(err)), err)


def select_tiles(tile_err_ptr, in_tiles_ptr, n_in, threshold, out_tiles_ptr, count_ptr, stream=0):
    """ptmi_select_tiles: of the candidates in_tiles_ptr[0..n_in) (uint32 tile indices; 0 = the tiles
    0..n_in themselves), those with tile_err[t] > threshold go to out_tiles_ptr in candidate order and
    their number to count_ptr[0] (uint32).  NaN and ties are dropped, +inf is kept; the two lists must
    not alias.  The rule is ptmi/error.py select_tiles_reference."""
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_select_tiles(_vp(tile_err_ptr), _vp(in_tiles_ptr), int(n_in), float(threshold),
                                            _vp(out_tiles_ptr), _vp(count_ptr), _vp(stream), err, len(err)), err)


def finalize_counts(sums_ptr, out_ptr, n_pixels, stream=0):
    """ptmi_finalize_counts: RGB = sum_c * (1.0 / n) with the pixel's own n = sums[4i+3] (0 where
    n == 0), A = 1.0.  The rule is ptmi/error.py finalize_counts_reference."""
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_finalize_counts(_vp(sums_ptr), _vp(out_ptr), int(n_pixels), _vp(stream), err, len(err)),
           err)


def denoise_work_bytes(width, height):
    """ptmi_denoise_work_bytes: the scratch ptmi_denoise needs for a W x H frame."""
    return load_library().ptmi_denoise_work_bytes(int(width), int(height))


def denoise_params(params=None):
    """A DenoiseParams from None (the defaults), a DenoiseParams or a dict of some of its fields."""
    return _params(DenoiseParams, params)


def denoise(rgba_ptr, se_ptr, feat_ptr, w, h, out_ptr, out_se_ptr=0, params=None, stream=0, work=None):
    """ptmi_denoise: the variance-guided a-trous filter over a W x H frame in device memory -- rgba_ptr
    (finalize), se_ptr (error_map) and feat_ptr (Scene.features) in, out_ptr (RGBA, must not alias
    rgba_ptr) and out_se_ptr (optional) out.  params: None, a DenoiseParams or a dict of its fields.
    The workspace is `work`, a torch tensor of at least denoise_work_bytes(w, h) bytes on the device, or
    one allocated here on torch's current stream.  The operation order is ptmi/denoise.py
    atrous_reference."""
    p = denoise_params(params)
    if work is None:
        import torch
        work = torch.empty(denoise_work_bytes(w, h) // 8, dtype=torch.float64, device="cuda")
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_denoise(_vp(rgba_ptr), _vp(se_ptr), _vp(feat_ptr), int(w), int(h), _ref(p), _vp(out_ptr),
                                       _vp(out_se_ptr), _vp(work.data_ptr()), work.numel() * work.element_size(),
                                       _vp(stream), err, len(err)), err)


def reproject_params(params=None):
    """A ReprojectParams from None (the defaults), a ReprojectParams or a dict of some of its fields."""
    return _params(ReprojectParams, params)


def _camera_record(prev_camera):
    if prev_camera is None:
        return None
    cam = np.ascontiguousarray(np.asarray(prev_camera).reshape(1))
    if cam.dtype.itemsize != layout.CAMERA_DTYPE.itemsize:
        raise TypeError("prev_camera: expected %d-byte records, got %d" % (layout.CAMERA_DTYPE.itemsize,
                                                                           cam.dtype.itemsize))
    return cam


def reproject(rgba_ptr, se_ptr, feat_ptr, prev_hist_ptr, prev_feat_ptr, prev_camera, w, h, out_hist_ptr,
              out_rgba_ptr=0, out_se_ptr=0, params=None, stream=0):
    """ptmi_reproject: temporal accumulation of a W x H frame in device memory -- this frame (rgba_ptr,
    se_ptr, feat_ptr) blended into the previous frame's history (prev_hist_ptr, W*H*HISTORY_DOUBLES;
    0 = first frame) found through prev_feat_ptr and prev_camera (the previous frame's camera record,
    host memory).  out_hist_ptr gets the new history (no output may overlap an input or another output), out_rgba_ptr /
    out_se_ptr (optional) the accumulated frame and its standard error, as denoise() takes them.
    params: None, a ReprojectParams or a dict of its fields.  The operation order is ptmi/temporal.py
    reproject_reference."""
    p = reproject_params(params)
    cam = _camera_record(prev_camera)
    err = ctypes.create_string_buffer(512)
    _check(load_library().ptmi_reproject(
        _vp(rgba_ptr), _vp(se_ptr), _vp(feat_ptr), _vp(prev_hist_ptr), _vp(prev_feat_ptr), _ptr(cam), int(w), int(h),
        _ref(p), _vp(out_hist_ptr), _vp(out_rgba_ptr), _vp(out_se_ptr), _vp(stream), err, len(err)), err)


def _object_records(objects, name):
    objs = np.ascontiguousarray(objects) if objects is not None else None
    if objs is not None and objs.dtype.itemsize != layout.OBJECT_DTYPE.itemsize:
        raise TypeError("%s: expected %d-byte records, got %d" % (name, layout.OBJECT_DTYPE.itemsize,
                                                                  objs.dtype.itemsize))
    return objs


def motion_table(prev_objects, cur_objects, motion_ptr, n_obj=None, stream=0):
    """ptmi_motion_table: how each object moved between two frames -- from the previous and the current
    object records (host arrays, the same objects in the same order) into motion_ptr, n_obj *
    MOTION_DOUBLES doubles of device memory, as reproject_motion takes them.  The arithmetic is
    ptmi/temporal.py motion_matrices.  Returns when the copy is done."""
    prev, cur = _object_records(prev_objects, "prev_objects"), _object_records(cur_objects, "cur_objects")
    if n_obj is None:
        if prev is None or cur is None or len(prev) != len(cur):
            raise ValueError("motion_table: two object lists of one length")
        n_obj = len(cur)
    err = ctypes.create_string_buffer(256)
    _check(load_library().ptmi_motion_table(_ptr(prev), _ptr(cur), int(n_obj), _vp(motion_ptr),
                                            _vp(stream), err, len(err)), err)


def reproject_motion(rgba_ptr, se_ptr, feat_ptr, prev_hist_ptr, prev_feat_ptr, prev_camera, w, h, out_hist_ptr,
                     motion_ptr, n_obj, out_rgba_ptr=0, out_se_ptr=0, params=None, stream=0):
    """ptmi_reproject_motion: reproject() for scenes whose objects move -- motion_ptr is the table
    motion_table() wrote for the previous and the current frame's objects, n_obj its length.  A pixel on
    a moved object looks its history up where that surface point was; with an all-static table the
    outputs are reproject()'s bit for bit.  The operation order is ptmi/temporal.py reproject_reference
    with `motion`."""
    p = reproject_params(params)
    cam = _camera_record(prev_camera)
    err = ctypes.create_string_buffer(512)
    _check(load_library().ptmi_reproject_motion(
        _vp(rgba_ptr), _vp(se_ptr), _vp(feat_ptr), _vp(prev_hist_ptr), _vp(prev_feat_ptr), _ptr(cam), int(w), int(h),
        _ref(p), _vp(out_hist_ptr), _vp(out_rgba_ptr), _vp(out_se_ptr), _vp(motion_ptr), int(n_obj), _vp(stream), err,
        len(err)), err)


def history_gather(rgba_ptr, se_ptr, feat_ptr, prev_hist_ptr, prev_feat_ptr, prev_camera, w, h, gathered_ptr,
                   motion_ptr=0, n_obj=0, params=None, stream=0):
    """ptmi_history_gather: reproject() -- or, with motion_ptr and n_obj, reproject_motion() -- up to the
    blend: gathered_ptr (W*H*HISTORY_DOUBLES) gets per pixel the history as found, (h_c, h_var, h_N, 0...),
    and (rgb, se^2, N = 0) where those calls would reset.  rectify() tests and blends it.  The operation
    order is ptmi/temporal.py gather_reference."""
    p = reproject_params(params)
    cam = _camera_record(prev_camera)
    err = ctypes.create_string_buffer(512)
    _check(load_library().ptmi_history_gather(
        _vp(rgba_ptr), _vp(se_ptr), _vp(feat_ptr), _vp(prev_hist_ptr), _vp(prev_feat_ptr), _ptr(cam), int(w), int(h),
        _ref(p), _vp(gathered_ptr), _vp(motion_ptr), int(n_obj), _vp(stream), err, len(err)), err)


def rectify_params(params=None):
    """A RectifyParams from None (the defaults), a RectifyParams or a dict of some of its fields."""
    return _params(RectifyParams, params)


def rectify(rgba_ptr, se_ptr, feat_ptr, gathered_ptr, w, h, out_hist_ptr, out_rgba_ptr=0, out_se_ptr=0, params=None,
            stream=0):
    """ptmi_rectify: the gathered history (history_gather) tested against this frame over a window of
    pixels on the same object, corrected by the offset found and blended as reproject() blends.
    out_hist_ptr gets (colour', var', N', rho, 0, 0) per pixel; out_rgba_ptr / out_se_ptr (optional) the
    accumulated frame and its standard error.  params: None, a RectifyParams or a dict of its fields.  The
    operation order is ptmi/temporal.py rectify_reference."""
    p = rectify_params(params)
    err = ctypes.create_string_buffer(512)
    _check(load_library().ptmi_rectify(
        _vp(rgba_ptr), _vp(se_ptr), _vp(feat_ptr), _vp(gathered_ptr), int(w), int(h), _ref(p), _vp(out_hist_ptr),
        _vp(out_rgba_ptr), _vp(out_se_ptr), _vp(stream), err, len(err)), err)


def variance_params(params=None):
    """A VarianceParams from None (the defaults), a VarianceParams or a dict of some of its fields."""
    return _params(VarianceParams, params)


def variance_estimate(rgba_ptr, se_ptr, feat_ptr, prev_mom_ptr, prev_feat_ptr, prev_camera, w, h, out_mom_ptr,
                      out_se_ptr, motion_ptr=0, n_obj=0, params=None, stream=0):
    """ptmi_variance_estimate: the standard error of a W x H frame's pixels estimated from the moments of each
    surface point's frames -- accumulated through history_gather()'s lookup (with motion_ptr and n_obj,
    reproject_motion()'s) on the previous frame's moment record (prev_mom_ptr, W*H*MOMENT_DOUBLES; 0 = first
    frame) -- or, where that history is too short, from a window of same-surface pixels of this frame.
    out_mom_ptr gets (mu', mu2', N', source, var, 0) per pixel and out_se_ptr sqrt(var), which reproject(),
    history_gather() + rectify() and denoise() take in the place of error_map()'s se; se_ptr (the map as
    rendered) may be 0.  params: None, a VarianceParams or a dict of its fields.  The operation order is
    ptmi/temporal.py variance_reference."""
    p = variance_params(params)
    cam = _camera_record(prev_camera)
    err = ctypes.create_string_buffer(512)
    _check(load_library().ptmi_variance_estimate(
        _vp(rgba_ptr), _vp(se_ptr), _vp(feat_ptr), _vp(prev_mom_ptr), _vp(prev_feat_ptr), _ptr(cam), int(w), int(h),
        _ref(p), _vp(out_mom_ptr), _vp(out_se_ptr), _vp(motion_ptr), int(n_obj), _vp(stream), err, len(err)), err)
