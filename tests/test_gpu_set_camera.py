"""ptmi_scene_set_camera on the GPU: after the call a resident scene renders, bit for bit, what a scene
freshly created with that camera renders -- sums, second moments, a tile-list render and the first-hit
records -- on the lockstep reference scene, on the reference scene switched between a pinhole and a
depth-of-field camera and to a non-affine one (the kernel instantiation changes in both directions), and
on the teapot mesh (tile classes, dispatch order).  Refused calls leave the scene as it was.

Frames: reference 36 x 20 at 8 spp, teapot 28 x 20 at 4 spp with explicit chunks (partial 8 x 8 tiles on
both axes); camera B is camera A orbited by 20 degrees."""
import numpy as np
import pytest

from ptmi import api, layout, temporal
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


def _fresh(records, cam, spp, chunks, rng=None, tiles=None):
    objs, tris, grps, _ = records
    sc = api.Scene(0, objs, tris, grps, cam)
    if rng is not None:
        sc.set_rng(rng)
    out, flags = _frame(sc, spp, chunks, tiles=tiles), sc.kernel_flags()
    sc.close()
    return out, flags


def _dof_camera(w, h):
    return temporal.orbit_camera(scene_inputs("reference", w, h, aperture=0.08, focal_length=1.6)[3], 20.0)


def _projective_camera(w, h):
    cam = temporal.orbit_camera(scene_inputs("reference", w, h)[3], 20.0)
    cam["inverse"][14] = 1e-3  # a bottom row other than (0, 0, 0, 1): the generic instantiation
    return cam


CASES = (("reference", 36, 20, 8, 0, None, None),
         ("reference", 36, 20, 8, 0, _dof_camera, None),
         ("reference", 36, 20, 8, 0, _projective_camera, None),
         ("teapot", 28, 20, 4, 2, None, [1, 5, 6, 10]))


@pytest.mark.parametrize("scene,w,h,spp,chunks,cam_b,tiles", CASES,
                         ids=("reference", "reference-dof", "reference-projective", "teapot"))
def test_set_camera_equals_a_fresh_scene(scene, w, h, spp, chunks, cam_b, tiles):
    records = scene_inputs(scene, w, h)
    cam_a = records[3]
    cam_b = cam_b(w, h) if cam_b else temporal.orbit_camera(cam_a, 20.0)
    want_a, flags_a = _fresh(records, cam_a, spp, chunks, tiles=tiles)
    want_b, flags_b = _fresh(records, cam_b, spp, chunks, tiles=tiles)
    assert not np.array_equal(want_a[0], want_b[0]) and not np.array_equal(want_a[2], want_b[2])
    sc = api.Scene(0, records[0], records[1], records[2], cam_a)
    first = _frame(sc, spp, chunks, tiles=tiles)
    assert _same(first, want_a) and sc.kernel_flags() == flags_a
    sc.set_camera(cam_b)
    assert sc.kernel_flags() == flags_b
    assert _same(_frame(sc, spp, chunks, tiles=tiles), want_b)
    sc.set_camera(cam_a)
    assert sc.kernel_flags() == flags_a
    assert _same(_frame(sc, spp, chunks, tiles=tiles), first)
    sc.close()
    print("%s: kernel flags A %d, B %d" % (scene, flags_a, flags_b))


def test_instantiation_follows_the_camera():
    """Aperture 0 <-> a depth-of-field camera, and an affine <-> a non-affine one: F_DOF (8) and F_PROJ (16)."""
    w, h = 36, 20
    objs, tris, grps, cam_a = scene_inputs("reference", w, h)
    sc = api.Scene(0, objs, tris, grps, cam_a)
    base = sc.kernel_flags()
    assert not base & (8 | 16)
    sc.set_camera(_dof_camera(w, h))
    assert sc.kernel_flags() & 8 and not sc.kernel_flags() & 16
    sc.set_camera(_projective_camera(w, h))
    assert sc.kernel_flags() & 16
    sc.set_camera(cam_a)
    assert sc.kernel_flags() == base
    sc.close()
    sc = api.Scene(0, objs, tris, grps, _dof_camera(w, h))  # and the other way round
    assert sc.kernel_flags() & 8
    sc.set_camera(cam_a)
    assert sc.kernel_flags() == base
    sc.close()


def test_mesh_tile_classes_follow_the_camera():
    """60 x 44: the smallest of the frames tried at which the 20-degree orbit changes a tile's class (three
    of 48 do; at 28 x 20 the teapot's twelve tiles keep theirs), still with partial tiles on both axes."""
    w, h, spp = 60, 44, 4
    records = scene_inputs("teapot", w, h)
    cam_a = records[3]
    cam_b = temporal.orbit_camera(cam_a, 20.0)
    sc = api.Scene(0, records[0], records[1], records[2], cam_a)
    _frame(sc, spp, 2)  # an ordered render: the classes and the dispatch order of view A are cached
    cost_a = sc.tile_cost()
    assert np.array_equal(cost_a, _tile_cost(records[0], records[1], records[2], cam_a, w, h).reshape(-1))
    sc.set_camera(cam_b)
    cost_b = sc.tile_cost()
    want_b = _tile_cost(records[0], records[1], records[2], cam_b, w, h).reshape(-1)
    print("tile classes A %s\ntile classes B %s" % (cost_a.tolist(), cost_b.tolist()))
    assert np.array_equal(cost_b, want_b)
    assert not np.array_equal(cost_a, want_b), "the two views have the same classes: the check shows nothing"
    sc.close()


def test_refused_cameras_leave_the_scene_as_it_was():
    w, h, spp = 36, 20, 8
    objs, tris, grps, cam_a = scene_inputs("reference", w, h)
    sc = api.Scene(0, objs, tris, grps, cam_a)
    first = _frame(sc, spp, 0)
    for bad in (scene_inputs("reference", w + 1, h)[3], scene_inputs("reference", w, h - 1)[3]):
        with pytest.raises(api.PtmiError) as e:
            sc.set_camera(bad)
        assert e.value.code == api.PTMI_ERR_ARG
    assert _same(_frame(sc, spp, 0), first)
    # the statistical mode: a non-affine camera is refused, a legal one equals a fresh scene in that mode
    sc.set_rng(api.RNG_XOSHIRO)
    stat_a = _frame(sc, spp, 0)
    flags = sc.kernel_flags()
    with pytest.raises(api.PtmiError) as e:
        sc.set_camera(_projective_camera(w, h))
    assert e.value.code == api.PTMI_ERR_UNSUPPORTED
    assert sc.kernel_flags() == flags and _same(_frame(sc, spp, 0), stat_a)
    cam_b = temporal.orbit_camera(cam_a, 20.0)
    want_b, flags_b = _fresh((objs, tris, grps, None), cam_b, spp, 0, rng=api.RNG_XOSHIRO)
    sc.set_camera(cam_b)
    assert sc.kernel_flags() == flags_b and _same(_frame(sc, spp, 0), want_b)
    assert not np.array_equal(want_b[0], stat_a[0])
    sc.close()
