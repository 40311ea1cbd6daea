"""ptmi_scene_set_objects on the GPU: after the call a resident scene renders, bit for bit, what a scene
freshly created with those objects renders -- sums, second moments, a tile-list render, the first-hit
records and the kernel instantiation -- and setting the first objects again restores the first frame.

Cases (reference scene 36 x 20 at 8 spp, teapot 28 x 20 at 4 spp with chunks = 2: partial 8 x 8 tiles on
both axes):
  translate   a scale+translate ball translated: sphere records, camera terms, the tiles' candidate masks
  rotate      a ball given a rotation: it leaves the scale+translate records (their number, the layout
              behind the camera record), then comes back; and a scene CREATED with the rotated ball gains a
              record when the rotation is taken away (the sphere and camera allocations grow)
  plane       the floor rotated about z so that row 1 of its inverse gets an x entry: n_planes_y, par
  material    a ball made reflective: the lockstep kernel <-> the material instantiation
  teapot      the mesh translated: the group's inverse, tile classes and dispatch order (the classes are
              checked at 60 x 44, the smallest frame at which tests/test_gpu_set_camera.py found they change)
Refused calls leave the scene rendering as before."""
import math

import numpy as np
import pytest

from ptmi import api, geom, layout, temporal
from tests.scene_inputs import scene_inputs
from tests.test_index_frame import _tile_cost

pytestmark = pytest.mark.gpu


def _frame(sc, spp, chunks, seed=11, tiles=None):
    """(sums, sq, features[, tile-list sums, tile-list sq]) of the scene as it stands, as numpy arrays."""
    import torch
    w, h = sc.width, sc.height
    kw = dict(dtype=torch.float64, device="cuda")
    seeds = torch.tensor(layout.seeds_go_float64(w * h, seed), **kw)
    sums, sq = torch.full((w * h * 4,), -1.0, **kw), torch.full((w * h,), -1.0, **kw)
    feat = torch.full((w * h * api.FEATURE_DOUBLES,), -7.0, **kw)
    sc.render_moments(spp, 0, spp, seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), chunks=chunks)
    sc.features(feat.data_ptr())
    out = [sums, sq, feat]
    if tiles is not None:
        t = torch.tensor(tiles, dtype=torch.int32, device="cuda")
        tsums, tsq = torch.full((w * h * 4,), -1.0, **kw), torch.full((w * h,), -1.0, **kw)
        sc.render_tiles(spp, 0, spp, t.data_ptr(), len(tiles), seeds.data_ptr(), tsums.data_ptr(), tsq.data_ptr(),
                        chunks=max(chunks, 1))
        out += [tsums, tsq]
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in out]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)) and len(a) == len(b)


def _fresh(objs, records, spp, chunks, rng=None, tiles=None):
    sc = api.Scene(0, objs, records[1], records[2], records[3])
    if rng is not None:
        sc.set_rng(rng)
    out, flags = _frame(sc, spp, chunks, tiles=tiles), sc.kernel_flags()
    sc.close()
    return out, flags


def _translated(objs, index=7):
    return temporal.move_object(objs, index, geom.translate(0.2, 0.05, -0.1))


def _rotated(objs, index=7):
    """The ball turned about its own centre: the same sphere, but its inverse leaves the scale+translate pattern."""
    t = [float(a) for a in objs[index]["transform"]]
    c = (t[3], t[7], t[11])
    m = geom.multiply(geom.translate(*c), geom.multiply(geom.rotate_z(math.radians(30.0)), geom.translate(-c[0], -c[1], -c[2])))
    return temporal.move_object(objs, index, m)


def _plane_rotated(objs, index=1):
    return temporal.move_object(objs, index, geom.rotate_z(math.radians(5.0)))


def _reflective(objs, index=7):
    out = objs.copy()
    out[index]["reflectivity"] = 0.6
    return out


CASES = (("reference", 36, 20, 8, 0, _translated, [0, 3, 7, 14]),
         ("reference", 36, 20, 8, 0, _rotated, [0, 3, 7, 14]),
         ("reference", 36, 20, 8, 0, _plane_rotated, [0, 3, 7, 14]),
         ("reference", 36, 20, 8, 0, _reflective, [0, 3, 7, 14]),
         ("teapot", 28, 20, 4, 2, lambda o: temporal.move_object(o, 6, geom.translate(0.15, 0.0, 0.1)), [1, 5, 6, 10]))
IDS = ("translate", "rotate", "plane", "material", "teapot")


@pytest.mark.parametrize("scene,w,h,spp,chunks,change,tiles", CASES, ids=IDS)
def test_set_objects_equals_a_fresh_scene(scene, w, h, spp, chunks, change, tiles):
    records = scene_inputs(scene, w, h)
    objs_a = records[0]
    objs_b = change(objs_a)
    want_a, flags_a = _fresh(objs_a, records, spp, chunks, tiles=tiles)
    want_b, flags_b = _fresh(objs_b, records, spp, chunks, tiles=tiles)
    assert not np.array_equal(want_a[0], want_b[0]), "the two object lists render alike: the check shows nothing"
    sc = api.Scene(0, objs_a, records[1], records[2], records[3])
    first = _frame(sc, spp, chunks, tiles=tiles)
    assert _same(first, want_a) and sc.kernel_flags() == flags_a
    sc.set_objects(objs_b)
    assert sc.kernel_flags() == flags_b
    assert _same(_frame(sc, spp, chunks, tiles=tiles), want_b)
    sc.set_objects(objs_a)
    assert sc.kernel_flags() == flags_a
    assert _same(_frame(sc, spp, chunks, tiles=tiles), first)
    sc.close()
    # and from the other side: a scene created with B (for `rotate`, with one scale+translate record fewer,
    # so that the way to A grows the sphere records and the allocation behind the camera record)
    sc = api.Scene(0, objs_b, records[1], records[2], records[3])
    sc.set_objects(objs_a)
    assert sc.kernel_flags() == flags_a and _same(_frame(sc, spp, chunks, tiles=tiles), want_a)
    sc.set_objects(objs_b)
    assert sc.kernel_flags() == flags_b and _same(_frame(sc, spp, chunks, tiles=tiles), want_b)
    sc.close()
    print("%s: kernel flags A %d, B %d" % (scene, flags_a, flags_b))


def test_cases_exercise_what_they_name():
    """The rotated ball's inverse leaves the scale+translate pattern, the rotated floor's row 1 gains an x
    entry, and the reflective ball changes the instantiation (F_MATERIALS = 4)."""
    w, h = 36, 20
    records = scene_inputs("reference", w, h)
    objs = records[0]
    inv = np.asarray(_rotated(objs)[7]["inverse"])
    assert inv[1] != 0.0 and inv[4] != 0.0 and np.asarray(objs[7]["inverse"])[1] == 0.0
    assert np.asarray(objs[1]["inverse"])[4] == 0.0 and np.asarray(_plane_rotated(objs)[1]["inverse"])[4] != 0.0
    sc = api.Scene(0, objs, records[1], records[2], records[3])
    base = sc.kernel_flags()
    assert not base & 4
    sc.set_objects(_reflective(objs))
    assert sc.kernel_flags() & 4
    sc.set_objects(objs)
    assert sc.kernel_flags() == base
    sc.close()


def test_a_set_camera_after_set_objects_sees_the_new_objects():
    """The two updates compose: objects B then camera B equals a fresh scene of both."""
    w, h, spp = 36, 20, 8
    records = scene_inputs("reference", w, h)
    objs_b, cam_b = _rotated(_translated(records[0]), 6), temporal.orbit_camera(records[3], 20.0)
    sc = api.Scene(0, objs_b, records[1], records[2], cam_b)
    want = _frame(sc, spp, 0)
    sc.close()
    sc = api.Scene(0, records[0], records[1], records[2], records[3])
    sc.set_objects(objs_b)
    sc.set_camera(cam_b)
    assert _same(_frame(sc, spp, 0), want)
    sc.set_camera(records[3])
    sc.set_objects(records[0])
    sc.set_camera(cam_b)
    sc.set_objects(objs_b)
    assert _same(_frame(sc, spp, 0), want)
    sc.close()


def test_mesh_tile_classes_follow_the_objects():
    w, h, spp = 60, 44, 4
    records = scene_inputs("teapot", w, h)
    objs_b = temporal.move_object(records[0], 6, geom.translate(0.25, 0.0, 0.0))
    sc = api.Scene(0, records[0], records[1], records[2], records[3])
    _frame(sc, spp, 2)  # an ordered render: the classes and the dispatch order of the first objects are cached
    cost_a = sc.tile_cost()
    sc.set_objects(objs_b)
    cost_b = sc.tile_cost()
    want_b = _tile_cost(objs_b, records[1], records[2], records[3], w, h).reshape(-1)
    print("tile classes A %s\ntile classes B %s" % (cost_a.tolist(), cost_b.tolist()))
    assert np.array_equal(cost_b, want_b)
    assert not np.array_equal(cost_a, want_b), "the two object lists have the same classes: the check shows nothing"
    sc.close()


def test_refused_objects_leave_the_scene_as_it_was():
    w, h, spp = 28, 20, 4
    records = scene_inputs("teapot", w, h)
    objs = records[0]
    sc = api.Scene(0, objs, records[1], records[2], records[3])
    first, flags = _frame(sc, spp, 2), sc.kernel_flags()
    other_type = objs.copy()
    other_type[7]["type"] = layout.TYPE_CUBE
    other_child = objs.copy()
    other_child[6]["children"][0] += 1
    other_count = objs.copy()
    other_count[6]["child_count"] = 0
    other_box = objs.copy()
    other_box[6]["bb_max"][1] *= 1.5
    for bad in (objs[:-1], np.concatenate([objs, objs[-1:]]), other_type, other_child, other_count, other_box):
        with pytest.raises(api.PtmiError) as e:
            sc.set_objects(bad)
        assert e.value.code == api.PTMI_ERR_ARG
    assert sc.kernel_flags() == flags and _same(_frame(sc, spp, 2), first)
    sc.close()
    # the statistical mode: a non-affine object is refused, a legal one equals a fresh scene in that mode
    w, h, spp = 36, 20, 8
    records = scene_inputs("reference", w, h)
    objs = records[0]
    sc = api.Scene(0, objs, records[1], records[2], records[3])
    sc.set_rng(api.RNG_XOSHIRO)
    stat_a, flags = _frame(sc, spp, 0), sc.kernel_flags()
    projective = objs.copy()
    projective[7]["inverse"][14] = 1e-3  # a bottom row other than (0, 0, 0, 1): the generic instantiation
    with pytest.raises(api.PtmiError) as e:
        sc.set_objects(projective)
    assert e.value.code == api.PTMI_ERR_UNSUPPORTED
    assert sc.kernel_flags() == flags and _same(_frame(sc, spp, 0), stat_a)
    objs_b = _translated(objs)
    want_b, flags_b = _fresh(objs_b, records, spp, 0, rng=api.RNG_XOSHIRO)
    sc.set_objects(objs_b)
    assert sc.kernel_flags() == flags_b and _same(_frame(sc, spp, 0), want_b)
    assert not np.array_equal(want_b[0], stat_a[0])
    sc.set_rng(api.RNG_NOISE3D)  # and outside that mode the projective object is a legal update
    want_p, flags_p = _fresh(projective, records, spp, 0)
    sc.set_objects(projective)
    assert sc.kernel_flags() == flags_p and flags_p & 16 and _same(_frame(sc, spp, 0), want_p)
    sc.close()
