"""The staged lockstep loop and the camera terms (ptmi_kernels.hip trace_lockstep;
find_closest_prims' CAM form) against a kernel that has neither.

The comparator is the one of test_gpu_lockstep: the same scene forced onto the material
instantiation (api.force_flags), which keeps the regeneration loop and computes every origin term
per ray.  Every comparison first asserts which instantiation each scene launches, so no kernel is
compared with itself, and that the image is not all zeros; then np.array_equal -- the stages and the
tables move work, never a bit.

The scenes are small (24x16, and 20x12 for edge tiles; 5 to 9 samples) and cover each form of
find_closest_prims that reads a table: the plane runs (floor / ceiling run, parallel pairs, the odd
plane), the scale+translate sphere forms (1, 2, 3, 4 spheres) beside the rotated sphere that keeps
the generic arithmetic, cylinders and cubes behind them, and cameras whose origin terms are special
(an exact zero; a first hit on the light).
"""
import numpy as np
import pytest

from ptmi import api, geom, layout, scenes, shapes
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu

F_CYLCUBE, F_MATERIALS, F_DOF, F_XRNG = 2, 4, 8, 64
SEED = 77


# ---- scenes -----------------------------------------------------------------------------------
def _camera(w, h, frm, to, ap=0.0):
    cam = scenes.Camera(w, h, scenes.PI_OVER_3, geom.point(*frm), geom.point(*to))
    cam.aperture, cam.focal_length = float(ap), 1.6 if ap else 0.0
    return cam


def _plane(*transforms, color=(0.9, 0.8, 0.7)):
    p = shapes.Plane()
    for t in transforms:
        p.set_transform(t)
    p.set_material(shapes.new_diffuse(*color))
    return p


def _ball(t, s, rot=None):
    sp = shapes.Sphere()
    sp.set_transform(geom.translate(*t))
    if rot is not None:
        sp.set_transform(rot)  # not a scale+translate inverse any more: the DevObject sphere loop
    sp.set_transform(geom.scale(*s))
    sp.set_material(shapes.new_diffuse(0.9, 0.8, 0.7))
    return sp


def _light():
    return scenes._light_sphere(geom.color(9, 9, 9))


def _records(objects, cam):
    objs, tris, grps = layout.build_scene_buffer_cl(objects)
    return objs, tris, grps, layout.camera_record(cam)


STD_FROM, STD_TO = (0, 0.1, -1.5), (0, 0.05, 0)
FLOOR = lambda: _plane(geom.translate(0, -.4, 0))  # noqa: E731
CEIL = lambda: _plane(geom.translate(0, .4, 0))  # noqa: E731
LEFT = lambda: _plane(geom.translate(-.6, 0, 0), geom.rotate_z(scenes.PI_OVER_2), color=(0.75, 0.25, 0.25))  # noqa: E731
RIGHT = lambda: _plane(geom.translate(.6, 0, 0), geom.rotate_z(scenes.PI_OVER_2), color=(0.25, 0.25, 0.75))  # noqa: E731
BACK = lambda: _plane(geom.translate(0, 0, .4), geom.rotate_x(scenes.PI_OVER_2))  # noqa: E731
TILT = lambda: _plane(geom.translate(0, -.3, 0), geom.rotate_z(0.3), geom.rotate_x(0.2))  # noqa: E731
BALLS = [((-0.35, -0.28, -0.15), (0.12, 0.12, 0.12)), ((0, -0.24, -0.30), (0.16, 0.16, 0.16)),
         ((0.3, -0.2, 0.1), (0.1, 0.2, 0.1))]

# plane lists: count, pairing and whether a floor / ceiling run leads the list (n_planes_y)
PLANES = {
    "1-y": [FLOOR], "1-wall": [BACK],
    "2-y-unpaired": [FLOOR, BACK], "2-walls-unpaired": [LEFT, BACK], "2-y-pair": [FLOOR, CEIL],
    "3-y-run": [FLOOR, CEIL, BACK], "3-walls": [LEFT, RIGHT, BACK], "3-tilted-first": [TILT, FLOOR, CEIL],
    "5-y-run": [FLOOR, CEIL, LEFT, RIGHT, BACK], "5-no-run": [LEFT, RIGHT, BACK, TILT, FLOOR],
}


def _plane_scene(name, w, h):
    return _records([_light()] + [f() for f in PLANES[name]] + [_ball(*BALLS[1])], _camera(w, h, STD_FROM, STD_TO))


def _sphere_scene(n_st, rotated, w, h):
    """n_st scale+translate spheres (the light is the first), optionally one rotated sphere."""
    objs = [_light(), FLOOR(), CEIL(), LEFT(), RIGHT(), BACK()] + [_ball(*b) for b in BALLS[:n_st - 1]]
    if rotated:
        objs.append(_ball((0.1, -0.1, -0.5), (0.1, 0.14, 0.08), rot=geom.rotate_y(0.7)))
    return _records(objs, _camera(w, h, STD_FROM, STD_TO))


def _cylcube_scene(w, h):
    cyl = shapes.Cylinder(0, 0.4, True)
    cyl.set_transform(geom.translate(0.35, -0.5, -0.2))
    cyl.set_transform(geom.scale(0.075, 1, 0.075))
    cyl.set_material(shapes.new_diffuse(0.92, 0.4, 0.8))
    cube = shapes.Cube()
    cube.set_transform(geom.translate(-0.3, -0.3, -0.3))
    cube.set_transform(geom.rotate_y(scenes.PI_OVER_4))
    cube.set_transform(geom.scale(0.1, 0.1, 0.06))
    cube.set_material(shapes.new_diffuse(0.25, 0.25, 0.75))
    objs = [_light(), FLOOR(), CEIL(), LEFT(), RIGHT(), BACK(), _ball(*BALLS[1]), cyl, cube]
    return _records(objs, _camera(w, h, STD_FROM, STD_TO))


def _reference(w, h, frm=STD_FROM, to=STD_TO, ap=0.0):
    objs, tris, grps, _ = scene_inputs("reference", w, h)
    return objs, tris, grps, layout.camera_record(_camera(w, h, frm, to, ap))


# ---- rendering --------------------------------------------------------------------------------
class Pair:
    """The scene on its own instantiation (staged, camera terms) and forced onto the material one."""

    def __init__(self, records, own=0, rng=None):
        import torch
        self.torch = torch
        self.new = api.Scene(0, *records)
        with api.force_flags(own | F_MATERIALS):
            self.old = api.Scene(0, *records)
        if rng is not None:
            self.new.set_rng(rng)
            self.old.set_rng(rng)
            own |= F_XRNG
        assert self.new.kernel_flags() == own, self.new.kernel_flags()
        assert self.old.kernel_flags() == (own | F_MATERIALS), self.old.kernel_flags()
        self.w, self.h = self.new.width, self.new.height
        self.seeds = torch.tensor(layout.seeds_go_float64(self.w * self.h, SEED), dtype=torch.float64, device="cuda")

    def sums(self, sc, spp, s0, s1, **kw):
        out = self.torch.empty(self.w * self.h * 4, dtype=self.torch.float64, device="cuda")
        sc.render(spp, s0, s1, self.seeds.data_ptr(), out.data_ptr(), **kw)
        return out

    def moments(self, sc, spp, s0, s1, **kw):
        out = self.torch.empty(self.w * self.h * 4, dtype=self.torch.float64, device="cuda")
        sq = self.torch.empty(self.w * self.h, dtype=self.torch.float64, device="cuda")
        sc.render_moments(spp, s0, s1, self.seeds.data_ptr(), out.data_ptr(), sq.data_ptr(), **kw)
        return out, sq

    def both(self, spp, s0=0, s1=None, **kw):
        s1 = spp if s1 is None else s1
        a, b = self.sums(self.new, spp, s0, s1, **kw), self.sums(self.old, spp, s0, s1, **kw)
        self.torch.cuda.synchronize()
        return a.cpu().numpy(), b.cpu().numpy()

    def close(self):
        self.new.close()
        self.old.close()


def _equal(a, b, what=""):
    assert np.array_equal(a, b), "%s: L-inf %.3e, %d values differ" % (what, np.nanmax(np.abs(a - b)), int((a != b).sum()))


def _check(a, b, count, what=""):
    assert np.any(a.reshape(-1, 4)[:, :3] != 0.0), "all-zero image " + what
    assert np.all(a[3::4] == count)
    _equal(a, b, what)


def _frame_and_paths(records, spp, own=0, rng=None, paths=True):
    """The spp-sample frame, then one-sample renders of every sample index: single paths."""
    p = Pair(records, own, rng)
    try:
        a, b = p.both(spp)
        _check(a, b, spp, "frame")
        if paths:
            lit = False
            for n in range(9):
                a, b = p.both(9, n, n + 1)
                assert np.all(a[3::4] == 1.0)
                _equal(a, b, "sample %d" % n)
                lit = lit or bool(np.any(a.reshape(-1, 4)[:, :3] != 0.0))
            assert lit, "every single-sample image is zero"
    finally:
        p.close()


# ---- tests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,spp", [(24, 16, 7), (20, 12, 5)])
def test_reference_scene_own_camera(w, h, spp):
    """20x12: edge tiles, whose lanes outside the image take no stage at all."""
    _frame_and_paths(_reference(w, h), spp)


def test_reference_scene_other_camera():
    """Another origin and orientation: every table entry differs from the standard camera's."""
    _frame_and_paths(_reference(24, 16, (0.3, 0.2, -1.2), (-0.1, -0.1, 0.1)), 9)


def test_camera_origin_on_the_floor_plane():
    """Origin y = -0.4 on the floor y = -0.4: the floor's origin term is 1 * -0.4 + 0.4, an exact zero
    (t = -0 / dy); its sign must stay unobservable."""
    _frame_and_paths(_reference(24, 16, (0, -0.4, -1.5), (0, 0.05, 0)), 7)


def test_camera_looking_at_the_light():
    """The path ends at b = 0 on the emissive sphere: record 0's colour rule in the first stage."""
    _frame_and_paths(_reference(24, 16, (0, 0.1, -1.5), (0, .399, 0)), 5)


@pytest.mark.parametrize("n_st,rotated", [(1, False), (2, False), (3, False), (4, False), (2, True), (3, True)])
def test_sphere_forms(n_st, rotated):
    """nq = 1, the peeled pair, pair + odd sphere, two pairs; a rotated sphere takes the DevObject loop
    with per-ray origin arithmetic beside the table-fed ones."""
    _frame_and_paths(_sphere_scene(n_st, rotated, 24, 16), 6, paths=(n_st == 3))


@pytest.mark.parametrize("name", sorted(PLANES))
def test_plane_forms(name):
    _frame_and_paths(_plane_scene(name, 20, 12), 6, paths=name in ("5-y-run", "3-tilted-first"))


def test_cylinders_and_cubes():
    """Instantiation <2>: the cylinder and cube loops follow the table-fed planes and spheres."""
    _frame_and_paths(_cylcube_scene(24, 16), 8, own=F_CYLCUBE)


def test_depth_of_field_stages_only():
    """<8>: the origin moves with the sample, so the first stage keeps the generic arithmetic; sample 0
    is the NaN ray (a dead path through every stage)."""
    _frame_and_paths(_reference(24, 16, ap=0.15), 9, own=F_DOF)


def test_statistical_rng():
    _frame_and_paths(_reference(24, 16), 8, rng=api.RNG_XOSHIRO)


def test_render_moments():
    """Colour sums equal render()'s; second moments equal the material kernel's."""
    p = Pair(_reference(20, 12))
    try:
        plain = p.sums(p.new, 9, 0, 9)
        s_new, q_new = p.moments(p.new, 9, 0, 9)
        s_old, q_old = p.moments(p.old, 9, 0, 9)
        p.torch.cuda.synchronize()
        plain, s_new, q_new, s_old, q_old = (t.cpu().numpy() for t in (plain, s_new, q_new, s_old, q_old))
        _check(s_new, plain, 9, "moment render's sums vs render")
        _equal(s_new, s_old, "sums")
        assert np.any(q_new != 0.0)
        _equal(q_new, q_old, "second moments")
    finally:
        p.close()


def test_sample_shard_and_chunked_tail():
    """A shard that starts at s0 > 0, and chunks = 3: every tile's 9 samples as three chunk items, whose
    stages start at n = c0 != 0."""
    p = Pair(_reference(24, 16))
    try:
        a, b = p.both(9, 4, 9)
        _check(a, b, 5, "shard [4, 9)")
        a, b = p.both(9, chunks=3)
        _check(a, b, 9, "chunks = 3")
        a, b = p.both(9, 2, 9, chunks=2)
        _check(a, b, 7, "shard [2, 9), chunks = 2")
    finally:
        p.close()


def test_two_live_scenes_keep_their_own_camera_terms():
    """Two scenes with different cameras alive at once, rendered alternately: the terms belong to the
    scene, so each keeps matching its own comparator."""
    p1 = Pair(_reference(24, 16))
    p2 = Pair(_reference(24, 16, (0.3, 0.2, -1.2), (-0.1, -0.1, 0.1)))
    try:
        first = None
        for _ in range(2):
            a1, b1 = p1.both(6)
            a2, b2 = p2.both(6)
            _check(a1, b1, 6, "scene 1")
            _check(a2, b2, 6, "scene 2")
            assert not np.array_equal(a1, a2)
            if first is None:
                first = (a1, a2)
        _equal(a1, first[0], "scene 1 again")
        _equal(a2, first[1], "scene 2 again")
    finally:
        p1.close()
        p2.close()
