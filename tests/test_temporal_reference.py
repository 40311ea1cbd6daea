"""Properties of the numpy statement of ptmi_reproject (ptmi/temporal.py reproject_reference) on CPU.
The first-hit records come from the brute-force comparator tests/features_ref.py (reference scene,
36 x 20); colours and standard errors are synthetic.

Bounds.  Equalities are asserted as equalities where the operation order makes them exact (resets,
the constant sequence, var at max_history = 1).  With an unchanged camera the reprojected place of a
pixel is its own centre up to the rounding of x_p = origin + t d and of T x_p (~1e-14 pixels), so the
neighbouring taps enter with weights of that size: the K-frame mean, its variance and N are asserted to
1e-9 (of the largest channel, relative, and of K), as the issue states them.  At max_history = 1 the
colour is h + 1 * (c - h): two roundings of values no larger than the frame's largest channel, asserted
to 1e-14 of it."""
import numpy as np
import pytest

from ptmi import temporal
from tests import features_ref
from tests.scene_inputs import scene_inputs

W, H = 36, 20
_cache = {}


def records(cam, scene="reference", w=W, h=H):
    """feat[h*w, 12] of `scene` seen through the camera record `cam`, by the brute-force comparator."""
    key = (scene, w, h, np.asarray(cam).tobytes())
    if key not in _cache:
        objs, tris, grps, _ = scene_inputs(scene, w, h)
        ref = features_ref.closest_hits(objs, tris, grps, cam, w, h)
        f = np.zeros((w * h, temporal.FEATURE_DOUBLES))
        f[:, 0:3], f[:, 3], f[:, 4:7], f[:, 7], f[:, 8:11] = ref["pos"], ref["t"], ref["normal"], ref["id"], ref["albedo"]
        _cache[key] = f
    return _cache[key]


def camera(w=W, h=H):
    return scene_inputs("reference", w, h)[3]


def frame(rng, w=W, h=H):
    rgba = np.ones((h * w, 4))
    rgba[:, :3] = rng.rand(h * w, 3) * 2.0
    return rgba.reshape(-1), 0.05 + rng.rand(h * w)


def test_first_frame_resets_every_pixel():
    rng = np.random.RandomState(1)
    rgba, se = frame(rng)
    rgba = rgba.reshape(-1, 4)
    rgba[5, 1], se[9], rgba[17, 0] = np.nan, np.inf, -np.inf
    feat = records(camera())
    hist, out, out_se = temporal.reproject_reference(rgba, se, feat, None, None, None, W, H)
    hist = hist.reshape(-1, 8)
    bad = np.zeros(W * H, dtype=bool)
    bad[[5, 9, 17]] = True
    assert np.all(hist[~bad, 4] == 1.0) and np.all(hist[bad, 4] == 0.0)
    assert np.array_equal(hist[:, 0:3], rgba[:, :3], equal_nan=True)
    assert np.array_equal(hist[:, 3], se * se) and np.all(hist[:, 5:] == 0.0)
    assert np.array_equal(out.reshape(-1, 4)[:, :3], rgba[:, :3], equal_nan=True) and np.all(out[3::4] == 1.0)
    assert np.array_equal(out_se, np.sqrt(se * se))


def test_constant_sequence_stays_constant_bit_for_bit():
    rng = np.random.RandomState(2)
    cam, feat = camera(), records(camera())
    rgba = np.ones((W * H, 4))
    rgba[:, :3] = (0.3, 0.7, 0.123456789)
    hist = None
    for k in range(4):
        se = 0.05 + rng.rand(W * H)
        hist, out, _ = temporal.reproject_reference(rgba, se, feat, hist, feat, cam, W, H)
        assert np.array_equal(out, rgba.reshape(-1)), k
        assert np.array_equal(hist.reshape(-1, 8)[:, :3], rgba[:, :3])
    hit = feat[:, 7] >= 0
    assert hit.any() and np.all(np.abs(hist.reshape(-1, 8)[hit, 4] - 4.0) <= 4e-9)


def test_unchanged_camera_accumulates_the_mean():
    rng = np.random.RandomState(3)
    K = 6
    cam, feat = camera(), records(camera()).copy()
    feat[40:60] = 0.0  # (the box is closed: some misses, as the feature pass writes them)
    feat[40:60, 7] = -1.0
    hit = feat[:, 7] >= 0
    frames = [frame(rng) for _ in range(K)]
    hist = None
    for rgba, se in frames:
        hist, out, out_se = temporal.reproject_reference(rgba, se, feat, hist, feat, cam, W, H, dict(max_history=K))
    hist = hist.reshape(-1, 8)
    mean = np.mean([f[0].reshape(-1, 4)[:, :3] for f in frames], axis=0)
    var = np.sum([f[1] ** 2 for f in frames], axis=0) / K ** 2
    scale = max(np.abs(f[0]).max() for f in frames)
    d_c = np.abs(hist[hit, :3] - mean[hit]).max() / scale
    d_v = (np.abs(hist[hit, 3] - var[hit]) / var[hit]).max()
    d_n = np.abs(hist[hit, 4] - K).max() / K
    print("K = %d: colour %.3e of the largest channel, variance %.3e relative, N %.3e relative" % (K, d_c, d_v, d_n))
    assert d_c <= 1e-9 and d_v <= 1e-9 and d_n <= 1e-9
    assert np.array_equal(out.reshape(-1, 4)[:, :3], hist[:, :3]) and np.array_equal(out_se, np.sqrt(hist[:, 3]))
    # a miss keeps no history: the last frame alone
    last = frames[-1]
    assert (~hit).any() and np.all(hist[~hit, 4] == 1.0)
    assert np.array_equal(hist[~hit, :3], last[0].reshape(-1, 4)[~hit, :3])
    # a longer sequence than max_history: N stops there
    for rgba, se in frames[:2]:
        hist2, _, _ = temporal.reproject_reference(rgba, se, feat, hist.reshape(-1), feat, cam, W, H, dict(max_history=K))
    assert np.abs(hist2.reshape(-1, 8)[hit, 4] - K).max() <= 1e-9 * K


def test_max_history_one_returns_the_current_frame():
    rng = np.random.RandomState(4)
    cam, feat = camera(), records(camera())
    (a, se_a), (b, se_b) = frame(rng), frame(rng)
    hist, _, _ = temporal.reproject_reference(a, se_a, feat, None, None, None, W, H)
    hist, out, out_se = temporal.reproject_reference(b, se_b, feat, hist, feat, cam, W, H, dict(max_history=1))
    hist = hist.reshape(-1, 8)
    assert np.all(hist[:, 4] == 1.0)
    assert np.array_equal(hist[:, 3], se_b * se_b)
    assert np.abs(out - b).max() <= 1e-14 * max(np.abs(a).max(), np.abs(b).max())


def test_orbit_resets_what_the_previous_view_did_not_show():
    """A 40-degree orbit.  The projection is recomputed here with numpy's own inverse; pixels within 1e-6
    pixels of a decision are left to the other tests."""
    rng = np.random.RandomState(5)
    cam_a = camera()
    cam_b = temporal.orbit_camera(cam_a, 40.0)
    feat_a, feat_b = records(cam_a), records(cam_b)
    (a, se_a), (b, se_b) = frame(rng), frame(rng)
    hist_a, _, _ = temporal.reproject_reference(a, se_a, feat_a, None, None, None, W, H)
    hist, _, _ = temporal.reproject_reference(b, se_b, feat_b, hist_a, feat_a, cam_a, W, H)
    hist = hist.reshape(-1, 8)
    hit = feat_b[:, 7] >= 0
    T = np.linalg.inv(np.asarray(cam_a["inverse"], dtype=np.float64).reshape(4, 4))
    pc = np.c_[feat_b[:, 0:3], np.ones(W * H)] @ T.T
    z = -pc[:, 2]
    with np.errstate(all="ignore"):
        fu = (cam_a["half_width"] - pc[:, 0] / z) / cam_a["pixel_size"] - 0.5
        fv = (cam_a["half_height"] - pc[:, 1] / z) / cam_a["pixel_size"] - 0.5
    eps = 1e-6
    behind = hit & (z < -eps)
    off = hit & (z > eps) & ((fu < -1 - eps) | (fu > W + eps) | (fv < -1 - eps) | (fv > H + eps))
    inside = hit & (z > eps) & (fu > eps) & (fu < W - 1 - eps) & (fv > eps) & (fv < H - 1 - eps)
    ids_a = feat_a[:, 7].reshape(H, W)
    x0, y0 = np.floor(np.where(inside, fu, 0)).astype(int), np.floor(np.where(inside, fv, 0)).astype(int)
    same = np.zeros(W * H, dtype=bool)
    for i, j in temporal.TAPS:
        same |= ids_a[np.minimum(y0 + j, H - 1), np.minimum(x0 + i, W - 1)] == feat_b[:, 7]
    other = inside & ~same
    print("40 degrees: %d hit pixels, %d behind, %d off the image, %d with four foreign taps, %d blended" %
          (hit.sum(), behind.sum(), off.sum(), other.sum(), (hist[:, 4] > 1.0).sum()))
    assert (behind | off).any() and other.any() and (hist[:, 4] > 1.0).any()
    for m in (behind, off, other, ~hit):
        assert np.all(hist[m, 4] == 1.0)
        assert np.array_equal(hist[m, :3], b.reshape(-1, 4)[m, :3]) and np.array_equal(hist[m, 3], (se_b * se_b)[m])
    # whatever blended took history from a tap of its own object
    assert np.all(same[(hist[:, 4] > 1.0) & inside])


def test_orbit_round_trip_and_composition():
    cam = camera()
    back = temporal.orbit_camera(temporal.orbit_camera(cam, 37.5), -37.5)
    assert np.abs(np.asarray(back["inverse"]) - np.asarray(cam["inverse"])).max() <= 1e-15
    for name in ("width", "height", "pixel_size", "half_width", "half_height", "aperture", "focal_length", "fov"):
        assert back[name] == cam[name]
    # the orbit keeps the camera's distance from the y axis and its height
    o0 = np.asarray(cam["inverse"]).reshape(4, 4)[:3, 3]
    o1 = np.asarray(temporal.orbit_camera(cam, 90.0)["inverse"]).reshape(4, 4)[:3, 3]
    assert abs(np.hypot(o0[0], o0[2]) - np.hypot(o1[0], o1[2])) <= 1e-12 and o0[1] == o1[1]


def test_cofactor_inverse_and_parameter_checks():
    m = np.asarray(temporal.orbit_camera(camera(), 12.0)["inverse"], dtype=np.float64)
    inv = temporal.cofactor_inverse(m).reshape(4, 4)
    assert np.abs(inv @ m.reshape(4, 4) - np.eye(4)).max() <= 1e-12
    with pytest.raises(ValueError):
        temporal.cofactor_inverse(np.zeros(16))
    for bad in (dict(max_history=0), dict(max_history=65537), dict(flags=1), dict(normal_cos=-1.0),
                dict(plane_dist=float("nan")), dict(min_weight=float("inf"))):
        with pytest.raises(ValueError):
            temporal.params_dict(bad)


@pytest.mark.parametrize("scene,w,h,step", (("reference", 36, 20, 0.0), ("reference", 36, 20, 3.0),
                                            ("reference", 36, 20, 40.0), ("teapot", 28, 20, 3.0)))
def test_few_decisions_hang_on_the_last_bits(scene, w, h, step):
    """The views of tests/test_gpu_reproject.py, three frames chained: the pixels the GPU comparison may
    leave out (temporal.undecided) stay within its cap of 1 % of a frame."""
    rng = np.random.RandomState(6)
    cam0 = scene_inputs(scene, w, h)[3]
    hist = prev_feat = prev_cam = None
    for k in range(3):
        cam = temporal.orbit_camera(cam0, k * step)
        feat = records(cam, scene, w, h)
        rgba, se = frame(rng, w, h)
        hist, _, _, info = temporal.reproject_reference(rgba, se, feat, hist, prev_feat, prev_cam, w, h, details=True)
        left_out = int(temporal.undecided(info, w, h).sum())
        print("%s step %g frame %d: %d of %d pixels undecided" % (scene, step, k, left_out, w * h))
        assert left_out <= 0.01 * w * h
        prev_feat, prev_cam = feat, cam
