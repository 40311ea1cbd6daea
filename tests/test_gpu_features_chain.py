"""The specular-chain feature pass (ptmi_scene_features_chain) on the GPU: against ptmi_scene_features bit
for bit where the first hit is final, against the numpy chain (tests/features_chain_ref.py) on the scenes of
planes and spheres, and against twin scenes through the library itself -- a planar mirror against the
hand-reflected scene behind it, thin glass against the scene without it.

Twin bounds.  The stated bounds allow EPS of path per chain step for a restart off the surface.  The pass
starts each segment at the hit point itself (no hit is taken at t <= EPS), so the unfolded ray is the twin's
ray and the bounds hold with room, on curved final surfaces as on planes; the two are reported apart because
a start beside the surface would show on the curved ones first (a turned normal)."""
import numpy as np
import pytest

from ptmi import api
from tests import features_chain_ref as fcr
from tests import features_ref
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu
EPS = fcr.EPS
_cache = {}


def _records(objs, tris, grps, cam, w, h, chain, rng=None, calls=1, **kw):
    import torch
    sc = api.Scene(0, objs, tris, grps, cam)
    if rng is not None:
        sc.set_rng(rng)
    out = []
    for _ in range(calls):
        feat = torch.full((w * h * api.FEATURE_DOUBLES,), -7.0, dtype=torch.float64, device="cuda")
        sc.features(feat.data_ptr(), chain=chain, **kw)
        torch.cuda.synchronize()
        out.append(feat.cpu().numpy().reshape(w * h, api.FEATURE_DOUBLES))
    sc.close()
    return out if calls > 1 else out[0]


def _scene(scene, w, h):
    """(first-hit records, chain records of two calls) of a named scene, traced once per frame."""
    key = (scene, w, h)
    if key not in _cache:
        inputs = scene_inputs(scene, w, h)
        _cache[key] = (_records(*inputs, w, h, False), _records(*inputs, w, h, True, calls=2))
    return _cache[key]


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("scene,w,h", (("reference", 64, 48), ("teapot", 44, 30)))
def test_scenes_without_specular_first_hits_keep_every_bit(scene, w, h):
    first, (chain, again) = _scene(scene, w, h)
    assert np.all(chain[:, 11] == 0.0)
    assert _same_bits(chain, first) and _same_bits(again, first)
    assert (first[:, 7] >= 0).any()


@pytest.mark.parametrize("scene,w,h", (("transparency", 64, 48), ("reflection", 64, 48),
                                       ("transparent_teapot", 44, 30)))
def test_first_hit_pixels_of_specular_scenes_keep_every_bit(scene, w, h):
    first, (chain, again) = _scene(scene, w, h)
    k = chain[:, 11]
    assert np.all(k == np.floor(k)) and np.all(k >= 0) and np.all(k <= 8)
    assert (k == 0).any() and (k >= 1).any()
    print("%s %dx%d: chain lengths %s" % (scene, w, h, np.bincount(k.astype(int)).tolist()))
    assert _same_bits(chain[k == 0], first[k == 0])
    assert _same_bits(chain, again), "two calls differ"
    other = _records(*scene_inputs(scene, w, h), w, h, True, rng=api.RNG_XOSHIRO)
    assert _same_bits(other, chain), "the RNG mode shows"
    # a record is a hit or a miss as a whole; the unfolded point lies on the camera ray, L along it
    hit = chain[:, 7] >= 0
    assert np.all(chain[~hit][:, :11] == np.where(np.arange(11) == 7, -1.0, 0.0))
    org, dirs = features_ref.camera_rays(scene_inputs(scene, w, h)[3], w, h)
    want = org + chain[hit][:, 3:4] * dirs[hit]
    assert np.abs(chain[hit][:, 0:3] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(np.linalg.norm(chain[hit][:, 4:7], axis=1) - 1.0).max() <= 1e-12 * 9
    assert np.all((chain[hit][:, 4:7] * dirs[hit]).sum(1) <= 0.0)


@pytest.mark.parametrize("scene", ("transparency", "reflection"))
def test_records_match_the_numpy_chain(scene):
    w, h = 64, 48
    _, (f, _) = _scene(scene, w, h)
    objs, _, _, cam = scene_inputs(scene, w, h)
    ref = fcr.chain(objs, cam, w, h)
    keep = ~ref["close"]
    left_out = int((~keep).sum())
    print("%s %dx%d: %d of %d pixels left out (comparator ties, s2 at 1)" % (scene, w, h, left_out, w * h))
    assert left_out <= 0.02 * w * h
    assert np.array_equal(f[keep][:, 7], ref["id"][keep].astype(np.float64))
    assert np.array_equal(f[keep][:, 11], ref["k"][keep].astype(np.float64))
    assert ref["k"][keep].max() >= 1
    hit = keep & (ref["id"] >= 0)
    tol = 1e-9 * (ref["k"][hit] + 1)
    dl = np.abs(f[hit][:, 3] - ref["L"][hit]) / ref["L"][hit]
    dx = np.abs(f[hit][:, 0:3] - ref["pos"][hit]).max(1) / np.maximum(1.0, np.abs(ref["pos"][hit]).max(1))
    dn = np.abs(f[hit][:, 4:7] - ref["normal"][hit]).max(1)
    print("max of error / (1e-9 (k + 1)): L %.3e, position %.3e, normal %.3e" %
          ((dl / tol).max(), (dx / tol).max(), (dn / tol).max()))
    assert np.all(dl <= tol) and np.all(dx <= tol) and np.all(dn <= tol)
    assert np.array_equal(f[hit][:, 8:11], ref["albedo"][hit])  # untextured finals: exact
    miss = keep & (ref["id"] < 0)
    assert np.all(f[miss][:, :7] == 0.0) and np.all(f[miss][:, 8:11] == 0.0)


def _mirror_twin():
    if "mirror" not in _cache:
        w, h = 64, 48
        mirror, twin, cam, to_mirror_id = fcr.planar_mirror_pair(w, h)
        _, tris, grps, _ = scene_inputs("reference", w, h)  # (no meshes: both empty)
        ref = features_ref.closest_hits(twin, tris, grps, cam, w, h)
        _cache["mirror"] = (_records(mirror, tris, grps, cam, w, h, True), _records(twin, tris, grps, cam, w, h, False),
                            to_mirror_id, np.array([int(o["type"]) == 0 for o in twin]), features_ref.decided(ref))
    return _cache["mirror"]


@pytest.mark.parametrize("finals", ("planes", "curved"))
def test_planar_mirror_shows_the_reflected_twin(finals):
    """The reference scene with a mirror for a back wall against the scene reflected by hand, both through the
    library: ids under the object mapping, position and L within 1e-9 relative plus EPS, normals within 1e-9.
    Left out: pixels where the twin's own first hit is a tie (features_ref.decided).

    Measured on an MI355X, 64 x 48: planes (658 pixels) max |dL| 2.416e-13, |dx| 2.416e-13, |dn| 1.225e-16;
    curved (74 pixels: the two spheres and the light in the mirror) max |dL| 2.709e-14, |dx| 2.620e-14, |dn| 6.192e-12."""
    chain, twin, to_mirror_id, is_plane, decided = _mirror_twin()
    m = (chain[:, 11] == 1.0) & decided
    assert set(np.unique(chain[:, 11])) == {0.0, 1.0} and m.sum() > 500
    assert np.array_equal(chain[m][:, 7], to_mirror_id(twin[m][:, 7]))
    sel = m & (is_plane[np.maximum(twin[:, 7].astype(int), 0)] == (finals == "planes"))
    assert sel.sum() >= 50
    a, b = chain[sel], twin[sel]
    dl = np.abs(a[:, 3] - b[:, 3])
    dx = np.abs(a[:, 0:3] - b[:, 0:3]).max(1)
    dn = np.abs(a[:, 4:7] - b[:, 4:7]).max()
    print("mirror twin, %s finals, %d pixels: max |dL| %.3e, |dx| %.3e, |dn| %.3e" % (finals, sel.sum(), dl.max(),
                                                                                     dx.max(), dn))
    assert np.array_equal(a[:, 8:11], b[:, 8:11])
    assert np.all(dl <= EPS + 1e-9 * b[:, 3])
    assert np.all(dx <= EPS + 1e-9 * np.maximum(1.0, np.abs(b[:, 0:3]).max(1)))
    assert dn <= 1e-9


def _glass_twin():
    if "glass" not in _cache:
        w, h = 44, 30
        objs, tris, grps, cam = scene_inputs("transparent_teapot", w, h)
        teapot = len(objs) - 1
        assert int(objs[teapot]["type"]) == 4 and float(objs[teapot]["refractive_index"]) == -1.0
        bare = (objs[:teapot].copy(), np.zeros(0, dtype=tris.dtype), np.zeros(0, dtype=grps.dtype), cam)
        _cache["glass"] = (teapot, _records(objs, tris, grps, cam, w, h, False),
                           _records(objs, tris, grps, cam, w, h, True, max_chain=16),
                           _records(*bare, w, h, False), _records(*bare, w, h, True, max_chain=16),
                           np.array([int(o["type"]) == 0 for o in bare[0]]))
    return _cache["glass"]


def test_thin_glass_shows_the_scene_behind_it():
    """transparent_teapot against the same scene without the teapot: where the chain only crossed the teapot
    (the first hit is the teapot, the chain ended on another object, and the twin's own chain is k == 0, so
    no mirror or glass ball lies on that line), the twin's first hit: same id and albedo, normals within 1e-9,
    position within k EPS plus 1e-9 relative.  The mesh is walked on every segment of these chains.

    Measured on an MI355X, 44 x 30: 108 pixels start on the teapot, 97 end behind it (k = 2 on 89, 3 on 5, 4 on 3);
    82 plane finals: max |dx| below 0.0005 k EPS (printed as 0.000), |dn| 0; 15 curved finals (the diffuse
    sphere): max |dx| below 0.0005 k EPS, |dn| 5.751e-14."""
    teapot, first, chain, twin, twin_chain, is_plane = _glass_twin()
    k = chain[:, 11]
    m = (first[:, 7] == teapot) & (chain[:, 7] != teapot) & (chain[:, 7] >= 0) & (twin_chain[:, 11] == 0.0)
    print("thin glass: %d pixels start on the teapot, %d end behind it; chain lengths %s" %
          ((first[:, 7] == teapot).sum(), m.sum(), np.bincount(k[m].astype(int)).tolist()))
    assert m.sum() >= 40 and k[m].min() >= 2  # in and out at the least
    a, b = chain[m], twin[m]
    plane = is_plane[np.maximum(b[:, 7].astype(int), 0)]
    dx = np.abs(a[:, 0:3] - b[:, 0:3]).max(1)
    dn = np.abs(a[:, 4:7] - b[:, 4:7]).max(1)
    for name, s in (("plane", plane), ("curved", ~plane)):
        if s.any():
            print("thin-glass twin, %s finals, %d pixels: max |dx| / (k EPS) %.3f, |dn| %.3e" %
                  (name, s.sum(), (dx / (k[m] * EPS))[s].max(), dn[s].max()))
    assert np.array_equal(a[:, 7], b[:, 7])
    assert np.array_equal(a[:, 8:11], b[:, 8:11])
    assert np.all(dx <= k[m] * EPS + 1e-9 * np.maximum(1.0, np.abs(b[:, 0:3]).max(1)))
    assert dn.max() <= 1e-9


def test_max_chain_one_stops_at_the_second_surface():
    w, h = 64, 48
    inputs = scene_inputs("transparency", w, h)
    _, (full, _) = _scene("transparency", w, h)
    one = _records(*inputs, w, h, True, max_chain=1)
    assert one[:, 11].max() == 1.0 and np.array_equal(one[:, 11] == 0.0, full[:, 11] == 0.0)
    assert _same_bits(one[full[:, 11] <= 1.0], full[full[:, 11] <= 1.0])
    # a pixel that would go on holds the second surface: for a glass ball entered from outside, the ball
    # itself from inside (ids 6 and 7), nearer than the full chain's final surface
    on = full[:, 11] >= 2.0
    ref = fcr.chain(inputs[0], inputs[3], w, h, max_chain=1)
    keep = on & ~ref["close"]
    assert keep.sum() > 100
    assert np.array_equal(one[keep][:, 7], ref["id"][keep].astype(np.float64))
    assert np.all(np.isin(one[keep][:, 7], (6.0, 7.0, 8.0)))
    assert np.abs(one[keep][:, 3] - ref["L"][keep]).max() <= 2e-9 * ref["L"][keep].max()
    assert np.all(one[keep][:, 3] < full[keep][:, 3])
