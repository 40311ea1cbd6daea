"""The first-hit feature pass (ptmi_scene_features) on the GPU: self-consistency of its records, and
the records against a brute-force numpy comparator (tests/features_ref.py: every object, every
triangle, no BVH).

Frames: reference 36 x 20, teapot 28 x 20 and the textured envmap scene 36 x 20 (synthetic images,
tests/textures_synth.py).  A pixel is left out of the comparison only when the comparator's own two
nearest candidates are within 1e-9 relative in t (silhouettes, ties); at most 1 % of a frame may be."""
import numpy as np
import pytest

import pyoracle
from ptmi import api, layout
from tests import features_ref, textures_synth
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu
FRAMES = (("reference", 36, 20), ("teapot", 28, 20), ("envmap", 36, 20))
_cache = {}


def _inputs(scene, w, h):
    return scene_inputs(scene, w, h), textures_synth.scene_textures(scene)


def _features(scene, w, h, rng=None):
    import torch
    (objs, tris, grps, cam), tex = _inputs(scene, w, h)
    sc = api.Scene(0, objs, tris, grps, cam, *(tex or ()))
    if rng is not None:
        sc.set_rng(rng)
    out = []
    for _ in range(2):
        feat = torch.full((w * h * api.FEATURE_DOUBLES,), -7.0, dtype=torch.float64, device="cuda")
        sc.features(feat.data_ptr())
        torch.cuda.synchronize()
        out.append(feat.cpu().numpy().reshape(w * h, api.FEATURE_DOUBLES))
    sc.close()
    return out


def _frame(scene, w, h):
    """The device records (two calls) and the comparator's, computed once per frame."""
    key = (scene, w, h)
    if key not in _cache:
        (objs, tris, grps, cam), tex = _inputs(scene, w, h)
        ref = features_ref.closest_hits(objs, tris, grps, cam, w, h, textures=tex, tex_sample=pyoracle.tex_sample,
                                        uv_maps=(pyoracle.spherical_map, pyoracle.cube_uv))
        _cache[key] = (_features(scene, w, h), ref)
    return _cache[key]


@pytest.mark.parametrize("scene,w,h", FRAMES)
def test_records_are_self_consistent(scene, w, h):
    (f, f2), ref = _frame(scene, w, h)
    assert np.array_equal(f, f2), "two calls differ"
    hit = f[:, 7] >= 0
    assert hit.any() and np.all(f[:, 11] == 0.0)
    assert np.all(f[~hit][:, 7] == -1.0) and np.all(np.delete(f[~hit], 7, axis=1) == 0.0)
    assert np.all(f[hit][:, 7] == np.floor(f[hit][:, 7]))
    n, x, t = f[hit][:, 4:7], f[hit][:, 0:3], f[hit][:, 3]
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-12
    org, dirs = ref["origin"], ref["dirs"][hit]  # the rays recomputed from the camera record in numpy
    assert np.all((n * (x - org)).sum(1) <= 0.0)
    want = org + t[:, None] * dirs
    assert np.abs(x - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.all(t > 1e-4) and np.all(t < 1024.0)


def test_records_do_not_depend_on_the_rng_mode():
    scene, w, h = FRAMES[0]
    (f, _), _ = _frame(scene, w, h)
    assert np.array_equal(_features(scene, w, h, rng=api.RNG_XOSHIRO)[0], f)


@pytest.mark.parametrize("scene,w,h", FRAMES)
def test_records_match_the_brute_force_comparator(scene, w, h):
    (f, _), ref = _frame(scene, w, h)
    keep = features_ref.decided(ref)
    left_out = int((~keep).sum())
    print("%s %dx%d: %d of %d pixels left out (comparator ties)" % (scene, w, h, left_out, w * h))
    assert left_out <= 0.01 * w * h
    assert np.array_equal(f[keep][:, 7], ref["id"][keep].astype(np.float64))
    hit = keep & (ref["id"] >= 0)
    dt = np.abs(f[hit][:, 3] - ref["t"][hit]) / ref["t"][hit]
    dx = np.abs(f[hit][:, 0:3] - ref["pos"][hit]).max(1) / np.maximum(1.0, np.abs(ref["pos"][hit]).max(1))
    dn = np.abs(f[hit][:, 4:7] - ref["normal"][hit]).max()
    print("max rel |dt| %.3e, rel |dx| %.3e, |dn| %.3e" % (dt.max(), dx.max(), dn))
    assert dt.max() <= 1e-9 and dx.max() <= 1e-9 and dn <= 1e-9
    plain, tex = hit & ~ref["textured"], hit & ref["textured"]
    assert np.array_equal(f[plain][:, 8:11], ref["albedo"][plain])
    if scene == "envmap":
        assert tex.any()
    if tex.any():  # the FP32 sampler: 1e-6
        da = np.abs(f[tex][:, 8:11] - ref["albedo"][tex]).max()
        print("textured albedo: max |diff| %.3e over %d pixels" % (da, int(tex.sum())))
        assert da <= 1e-6
