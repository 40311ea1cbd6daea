"""Properties of the numpy statement of the specular chain (tests/features_chain_ref.py), on CPU: it is
the comparator of tests/test_gpu_features_chain.py, so what it states is checked here against
tests/features_ref.py and against the optics it restates."""
import math

import numpy as np
import pytest

from ptmi import geom, layout, shapes
from tests import features_chain_ref as fcr
from tests import features_ref
from tests.scene_inputs import scene_inputs

W, H = 44, 30


def test_first_hit_pixels_equal_the_first_hit_comparator():
    """The reference scene has no specular surface: every pixel has k == 0 and features_ref's record."""
    objs, tris, grps, cam = scene_inputs("reference", W, H)
    ref, ch = features_ref.closest_hits(objs, tris, grps, cam, W, H), fcr.chain(objs, cam, W, H)
    assert np.all(ch["k"] == 0) and len(ch["steps"]) == 1
    assert np.array_equal(ch["id"], ref["id"])
    hit = ref["id"] >= 0
    assert hit.any() and np.all(ch["L"][~hit] == 0.0) and np.all(ch["pos"][~hit] == 0.0)
    assert np.abs(ch["L"] - ref["t"])[hit].max() <= 1e-12
    assert np.abs(ch["pos"] - ref["pos"])[hit].max() <= 1e-12
    assert np.abs(ch["normal"] - ref["normal"])[hit].max() <= 1e-12
    assert np.array_equal(ch["albedo"], ref["albedo"])
    assert np.array_equal(ch["close"], ~features_ref.decided(ref))


def test_specular_scenes_keep_the_first_hit_where_it_is_final():
    for scene in ("transparency", "reflection"):
        objs, tris, grps, cam = scene_inputs(scene, W, H)
        ref, ch = features_ref.closest_hits(objs, tris, grps, cam, W, H), fcr.chain(objs, cam, W, H)
        k0 = ch["k"] == 0
        assert k0.any() and (~k0).any()
        assert np.array_equal(ch["id"][k0], ref["id"][k0]) and np.array_equal(ch["albedo"][k0], ref["albedo"][k0])
        assert np.abs(ch["pos"] - ref["pos"])[k0].max() <= 1e-12
        first = ch["steps"][0]["id"]  # a chain starts where the first hit is a mirror or glass
        refl = np.array([o["reflectivity"] >= 0.5 or o["refractive_index"] != 1.0 for o in objs])
        assert np.array_equal(~k0, (first >= 0) & refl[np.maximum(first, 0)])


def test_planar_mirror_records_equal_the_reflected_twin():
    mirror, twin, cam, to_mirror_id = fcr.planar_mirror_pair(W, H)
    none = np.zeros(0)
    ch = fcr.chain(mirror, cam, W, H)
    ref = features_ref.closest_hits(twin, none, none, cam, W, H)
    m = (ch["k"] == 1) & ~ch["close"] & features_ref.decided(ref)
    assert set(np.unique(ch["k"])) == {0, 1} and m.sum() > 0.2 * W * H
    assert np.all(ch["steps"][0]["id"][ch["k"] == 1] == fcr.BACK_WALL)
    assert np.array_equal(ch["id"][m], to_mirror_id(ref["id"][m]))
    assert len(np.unique(ch["id"][m])) >= 5  # the light, walls and both spheres show in the mirror
    # A segment starts at the hit point itself, so the unfolded ray is the twin's ray: rounding only, also
    # where the final surface is curved (the light's rim has a radius of curvature of 3.5e-4).
    plane = np.array([int(o["type"]) == 0 for o in twin])[np.maximum(ref["id"], 0)]
    assert (m & plane).any() and (m & ~plane).any()
    assert np.abs(ch["L"] - ref["t"])[m].max() <= 1e-9 and np.abs(ch["pos"] - ref["pos"])[m].max() <= 1e-9
    assert np.abs(ch["normal"] - ref["normal"])[m].max() <= 1e-9
    assert np.array_equal(ch["albedo"][m], ref["albedo"][m])


def test_snells_law_at_a_glass_spheres_first_interface():
    objs, _, _, cam = scene_inputs("transparency", W, H)
    ch = fcr.chain(objs, cam, W, H)
    s0 = ch["steps"][0]
    glass = (s0["rule"] == fcr.REFRACT)
    assert glass.sum() > 20 and set(np.unique(s0["id"][glass])) == {6, 7}
    for k in (6, 7):
        g = glass & (s0["id"] == k)
        ri = float(objs[k]["refractive_index"])
        d_in, d_out, n = ch["dirs"][g], s0["rd_out"][g], s0["normal"][g]
        assert np.abs(np.linalg.norm(d_out, axis=1) - 1.0).max() <= 1e-12
        sin_i = np.linalg.norm(np.cross(d_in, n), axis=1)
        sin_t = np.linalg.norm(np.cross(d_out, n), axis=1)
        assert np.abs(sin_i - ri * sin_t).max() <= 1e-12
        assert np.all((d_out * n).sum(1) < 0.0)  # it goes in
        assert np.abs((np.cross(d_in, n) * d_out).sum(1)).max() <= 1e-12  # in the plane of incidence
        assert np.allclose(s0["s2"][g], (sin_i / ri) ** 2, rtol=0, atol=1e-12)
    # the second interface is met from inside: nr = ri there, and the ray leaves the sphere
    s1 = ch["steps"][1]
    back = np.isin(s1["idx"], np.flatnonzero(glass))
    assert np.all(np.isin(s1["rule"][back], (fcr.REFRACT, fcr.TIR)))


def _plane(transforms, material):
    p = shapes.Plane()
    for t in transforms:
        p.set_transform(t)
    p.set_material(material)
    return p


def test_total_internal_reflection_takes_the_reflect_branch():
    """Down through a glass slab's top face (y = 0, normal incidence: straight on, inside), onto a glass
    face tilted by 60 degrees: 1.5^2 sin^2 60 = 1.6875 > 1, so the ray is reflected, tinted, and still inside."""
    glass = shapes.Material(geom.tuple3(0.5, 1.0, 0.25), geom.tuple3(0, 0, 0), 1.5, 0.0)
    top = _plane([], glass)
    tilted = _plane([geom.translate(0, -1, 0), geom.rotate_z(math.pi / 3)], glass)
    walls = [_plane([geom.translate(x, 0, 0), geom.rotate_z(math.pi / 2)], shapes.new_diffuse(0.2, 0.4, 0.6))
             for x in (-50, 50)]
    objs, _, _ = layout.build_scene_buffer_cl([top, tilted] + walls)
    ch = fcr.chain_rays(objs, [[0.0, 1.0, 0.0]], [[0.0, -1.0, 0.0]], max_chain=2)
    s0, s1, s2 = ch["steps"]
    assert s0["id"][0] == 0 and s0["rule"][0] == fcr.REFRACT and np.allclose(s0["rd_out"][0], (0, -1, 0), atol=1e-15)
    assert s1["id"][0] == 1 and s1["rule"][0] == fcr.TIR and s1["s2"][0] == pytest.approx(1.6875, abs=1e-12)
    n = s1["normal"][0]
    assert np.allclose(s1["rd_out"][0], np.array([0, -1.0, 0]) + 2.0 * n[1] * n, atol=1e-15)
    assert abs(np.linalg.norm(s1["rd_out"][0]) - 1.0) <= 1e-15
    # k == max_chain: the third hit is final whatever it is; its albedo carries the reflection's tint only
    assert ch["k"][0] == 2 and s2["rule"][0] == fcr.FINAL
    c_final = np.asarray(objs[s2["id"][0]]["color"][:3], dtype=np.float64)
    assert np.allclose(ch["albedo"][0], np.array([0.5, 1.0, 0.25]) * c_final, atol=0)
    assert ch["L"][0] == pytest.approx(s0["t"][0] + s1["t"][0] + s2["t"][0], abs=1e-15)
    # the unfolded normal: U = I - 2 n n^T applied to the final normal, facing the first ray
    un = s2["normal"][0] - 2.0 * n * (n @ s2["normal"][0])
    un = -un if un[1] < 0 else un  # rd0 = (0, -1, 0)
    assert np.allclose(ch["normal"][0], un, atol=1e-15)
