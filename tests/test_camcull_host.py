"""The camera-ray stage's candidate masks (csrc/ptmi_camcull.h) from the classifier's host build
(ptmi_diag_tile_cull_host: no device call) against a brute force over every tile's footprint
(tests/camcull_ref.py: 17 x 17 rays per tile, corners and edges included, numpy doubles).

Hard condition: no ray of a tile records an object whose bit the tile's mask clears.  Non-vacuity: a bit
kept on a tile where the brute force finds no candidate has a candidate within one tile.  Cases: the
reference scene at 160 x 120 with its own camera, one outside the box and one on the floor plane (an exact
zero origin term), 100 x 75 (edge tiles classified by their full 8 x 8 footprint), and plane / sphere scenes
of tests/test_gpu_stages.py (tilted planes, an ellipsoid, a rotated sphere whose bit does not exist).
"""
import numpy as np
import pytest

from ptmi import api
from tests import camcull_ref as ref

CASES = ref.host_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cleared_bits_are_candidate_free_and_kept_bits_are_near_a_candidate(name):
    objs, tris, grps, cam = CASES[name]
    masks = api.tile_cull_host(objs, tris, grps, cam)
    cleared, loose = ref.check_masks(masks, objs, cam)
    print("%s: %d bits cleared, %d kept on candidate-free tiles; planes kept %s, spheres kept %s"
          % ((name, cleared, loose) + ref.plane_counts(masks, objs)))
    assert cleared > 0, "nothing culled"


def test_reference_view_keeps_what_the_issue_expects():
    """The flagship view: most tiles keep three planes and no sphere; no tile keeps fewer than the back wall
    and one plane of each pair."""
    objs, tris, grps, cam = CASES["reference-160x120"]
    masks = api.tile_cull_host(objs, tris, grps, cam)
    planes, spheres = ref.plane_counts(masks, objs)
    assert min(planes) >= 3 and planes[3] > sum(planes.values()) // 2, planes
    assert spheres.get(0, 0) > sum(spheres.values()) // 3, spheres


def test_edge_tiles_use_the_full_footprint():
    """100 x 75: 13 x 10 tiles; the last column and row reach past the image.  Their masks are those of a
    104 x 80 frame with the same pixel mapping (the record's width and height alone changed), whose tiles
    are all whole -- and the brute force above samples the full 8 x 8 footprint of every tile."""
    objs, tris, grps, cam = CASES["reference-100x75"]
    masks = api.tile_cull_host(objs, tris, grps, cam)
    assert masks.shape == (13 * 10,)
    whole = np.array(cam).copy()
    whole["width"], whole["height"] = 104, 80
    assert np.array_equal(masks, api.tile_cull_host(objs, tris, grps, whole))


def test_sixteen_objects_and_buffer_size():
    objs, tris, grps, cam = ref.many_planes(64, 48)
    masks = api.tile_cull_host(objs, tris, grps, cam)
    ref.check_masks(masks, objs, cam)
    out = np.zeros(3, dtype=np.uint32)
    lib = api.load_library()
    import ctypes
    err = ctypes.create_string_buffer(256)
    o, t, g, c = api._records(objs, tris, grps, cam)
    rc = lib.ptmi_diag_tile_cull_host(api._ptr(o), len(o), api._ptr(t), len(t), api._ptr(g), len(g), api._ptr(c),
                                      out.ctypes.data_as(ctypes.c_void_p), len(out), err, len(err))
    assert rc != 0 and b"tiles" in err.value
