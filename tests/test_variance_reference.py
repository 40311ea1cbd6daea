"""Properties of the numpy statement of ptmi_variance_estimate (ptmi/temporal.py variance_reference) on CPU.
The first-hit records come from the brute-force comparator tests/features_ref.py; colours are synthetic.

Bounds.  Equalities are asserted as equalities where the operation order makes them exact (the constant
sequence, the resets, the sources, an all-static motion table).  The two unbiasedness checks compare the mean over
pixels of the estimated variance with the known 3 sigma^2 (the sum over the three channels) and allow 6 standard
errors of that mean, computed from the sample of per-pixel estimates itself: the estimates are unbiased by their
N / (N - 1) factors, and a 6-sigma excursion of a mean of hundreds of pixels has probability ~2e-9.  With an
unchanged camera the neighbouring taps enter the lookup with weights ~1e-14 (tests/test_temporal_reference.py),
which moves nothing at that scale."""
import numpy as np
import pytest

from ptmi import temporal
from tests.scene_inputs import scene_inputs
from tests.test_temporal_reference import camera, records

W, H = 36, 20
SIGMA = 0.25


def plane_records(w, h):
    """One plane facing the camera: every pixel a hit on object 0 with the same normal (the reference scene's
    camera; the positions are the pixels' rays at depth 5, so a static camera reprojects each onto itself)."""
    from tests import features_ref
    cam = camera(w, h)
    org, dirs = features_ref.camera_rays(cam, w, h)
    fwd = dirs.mean(0) / np.linalg.norm(dirs.mean(0))
    t = 5.0 / (dirs @ fwd)
    f = np.zeros((w * h, temporal.FEATURE_DOUBLES))
    f[:, 0:3], f[:, 3], f[:, 4:7], f[:, 7] = org + dirs * t[:, None], t, -fwd, 0.0
    return cam, f


def noise_frame(rng, w, h, mean=(0.6, 0.9, 0.4)):
    rgba = np.ones((h * w, 4))
    rgba[:, :3] = np.asarray(mean) + SIGMA * rng.randn(h * w, 3)
    return rgba.reshape(-1)


def test_constant_sequence_has_zero_variance_bit_for_bit():
    """A moving camera (1.5 degrees per frame): the taps' weights are anything, the moments stay exact."""
    cam0 = camera()
    rgba = np.ones((W * H, 4))
    rgba[:, :3] = (0.3, 0.7, 0.123456789)
    s = (0.3 * 0.3 + 0.7 * 0.7) + 0.123456789 * 0.123456789
    mom = prev_feat = prev_cam = None
    for k in range(6):
        cam = temporal.orbit_camera(cam0, 1.5 * k)
        feat = records(cam)
        mom, se = temporal.variance_reference(rgba, None, feat, mom, prev_feat, prev_cam, W, H, dict(min_count=2))
        m = mom.reshape(-1, 8)
        assert np.array_equal(m[:, 0:3], rgba[:, :3]) and np.all(m[:, 3] == s), k
        # (a pixel alone on its surface has no second tap: the fallback, whose s is no estimate from the sequence)
        est = m[:, 5] != 3.0
        assert est.mean() > 0.95 and np.all(m[:, 7] == 0.0), k
        assert np.all(m[est, 6] == 0.0) and np.all(se[est] == 0.0), k
        assert np.all(m[~est, 6] == s) and np.all(m[~est, 4] < 4.0), k
        prev_feat, prev_cam = feat, cam
    hit = feat[:, 7] >= 0
    assert (m[hit, 4] > 4.0).mean() > 0.8 and (m[hit, 5] == 1.0).mean() > 0.8, "the history grew under the orbit"


def _within_six_standard_errors(v, label):
    mean, sem = v.mean(), v.std(ddof=1) / np.sqrt(v.size)
    print("%s: mean variance %.6f over %d pixels, expected %.6f, standard error %.6f (%.2f of them off)" %
          (label, mean, v.size, 3 * SIGMA ** 2, sem, (mean - 3 * SIGMA ** 2) / sem))
    assert abs(mean - 3 * SIGMA ** 2) <= 6.0 * sem


def test_temporal_estimate_is_unbiased():
    rng = np.random.RandomState(11)
    cam, feat = plane_records(W, H)
    mom = None
    for k in range(8):
        mom, se = temporal.variance_reference(noise_frame(rng, W, H), None, feat, mom, feat, cam, W, H,
                                              dict(max_history=64, min_temporal=2))
        m = mom.reshape(-1, 8)
        assert np.abs(m[:, 4] - (k + 1)).max() <= 1e-9 * (k + 1), "N' stays below max_history"
        if k + 1 >= 3:  # (N' is k + 1 up to ~1e-14: at k + 1 = min_temporal a pixel may go either way)
            assert np.all(m[:, 5] == 1.0)
            assert np.array_equal(se, np.sqrt(m[:, 6]))
            _within_six_standard_errors(m[:, 6], "temporal, %d frames" % (k + 1))


def test_spatial_estimate_is_unbiased():
    rng = np.random.RandomState(12)
    w, h = 48, 40
    cam, feat = plane_records(w, h)
    for radius in (1, 3, 4):
        mom, se = temporal.variance_reference(noise_frame(rng, w, h), None, feat, None, None, None, w, h,
                                              dict(radius=radius))
        m = mom.reshape(h, w, 8)
        assert np.all(m[..., 4] == 1.0)
        assert np.all(m[radius:h - radius, radius:w - radius, 5] == 2.0)
        inner = m[radius:h - radius, radius:w - radius, 6].reshape(-1)  # (full windows)
        # a window's estimate shares taps with its neighbours': take every (2 radius + 1)-th pixel both ways
        # so that the sample's own standard error holds
        sparse = m[radius:h - radius:2 * radius + 1, radius:w - radius:2 * radius + 1, 6].reshape(-1)
        _within_six_standard_errors(sparse, "spatial, radius %d" % radius)
        assert abs(inner.mean() - 3 * SIGMA ** 2) <= 0.1 * 3 * SIGMA ** 2


def test_sources_follow_min_temporal_and_min_count():
    rng = np.random.RandomState(13)
    cam, feat = plane_records(W, H)
    se_in = 0.05 + rng.rand(W * H)
    for min_temporal in (2, 3, 5):
        mom = None
        for k in range(6):
            rgba = noise_frame(rng, W, H)
            mom, se = temporal.variance_reference(rgba, se_in, feat, mom, feat, cam, W, H,
                                                  dict(min_temporal=min_temporal, min_count=100))
            m = mom.reshape(-1, 8)
            # (N' is k + 1 up to ~1e-14: the frame at which it reaches min_temporal may go either way)
            if k + 1 < min_temporal:
                assert np.all(m[:, 5] == 3.0), "min_count above (2 radius + 1)^2: the fallback everywhere early"
                assert np.array_equal(m[:, 6], se_in * se_in) and np.array_equal(se, np.sqrt(se_in * se_in))
            elif k + 1 > min_temporal:
                assert np.all(m[:, 5] == 1.0)
    # without se the fallback is the pixel's own magnitude; a non-finite se_p falls back to it too
    rgba = noise_frame(rng, W, H)
    c = rgba.reshape(-1, 4)[:, :3]
    s = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    mom, se = temporal.variance_reference(rgba, None, feat, None, None, None, W, H, dict(min_count=100))
    assert np.all(mom.reshape(-1, 8)[:, 5] == 3.0) and np.array_equal(mom.reshape(-1, 8)[:, 6], s)
    se_inf = se_in.copy()
    se_inf[::3] = np.inf
    mom, se = temporal.variance_reference(rgba, se_inf, feat, None, None, None, W, H, dict(min_count=100))
    assert np.array_equal(mom.reshape(-1, 8)[:, 6], np.where(np.isfinite(se_inf), se_inf * se_inf, s))
    # min_count within reach: spatial inside, and the count decides at the image's corners
    mom, _ = temporal.variance_reference(rgba, None, feat, None, None, None, W, H, dict(radius=1, min_count=5))
    src = mom.reshape(H, W, 8)[..., 5]
    assert np.all(src[1:-1, :] == 2.0) and np.all(src[:, 1:-1] == 2.0)
    assert src[0, 0] == 3.0 and src[0, -1] == 3.0 and src[-1, 0] == 3.0 and src[-1, -1] == 3.0  # (4 taps)


def test_non_finite_pixels_and_a_frame_of_misses():
    rng = np.random.RandomState(14)
    cam, feat = plane_records(W, H)
    rgba = noise_frame(rng, W, H).reshape(-1, 4)
    bad = [5, W + 7, 3 * W + 2]
    rgba[bad[0], 1], rgba[bad[1], 0], rgba[bad[2], 2] = np.nan, np.inf, -np.inf
    se_in = 0.05 + rng.rand(W * H)
    for se_arg in (se_in, None):
        mom, se = temporal.variance_reference(rgba, se_arg, feat, None, None, None, W, H)
        m = mom.reshape(-1, 8)
        assert np.all(m[bad, 4] == 0.0) and np.all(m[bad, 5:] == 0.0)
        assert np.array_equal(m[bad, 0:3], rgba[bad, :3], equal_nan=True)
        assert np.array_equal(se[bad], se_in[bad] if se_arg is not None else np.full(3, np.inf))
        ok = np.ones(W * H, dtype=bool)
        ok[bad] = False
        assert np.all(m[ok, 4] == 1.0) and np.isfinite(m[ok]).all() and np.isfinite(se[ok]).all()
    # no later frame reads such a pixel: the next frame is finite everywhere, and around the bad pixels N' < 2
    nxt, se2 = temporal.variance_reference(noise_frame(rng, W, H), None, feat, mom, feat, cam, W, H)
    n2 = nxt.reshape(-1, 8)
    assert np.isfinite(n2).all() and np.isfinite(se2).all()
    assert np.all(n2[bad, 4] == 1.0) and (n2[:, 4] > 1.5).sum() >= W * H - 3 * 9
    # a frame of misses only: no history, the window pools the misses
    miss = np.zeros((W * H, temporal.FEATURE_DOUBLES))
    miss[:, 7] = -1.0
    a, _ = temporal.variance_reference(noise_frame(rng, W, H), None, miss, None, None, None, W, H)
    b, se_b = temporal.variance_reference(noise_frame(rng, W, H), None, miss, a, miss, cam, W, H)
    b = b.reshape(-1, 8)
    assert np.all(b[:, 4] == 1.0) and np.all(b[:, 5] == 2.0) and np.isfinite(se_b).all()
    # a NaN id matches nothing, itself included: the fallback
    odd = feat.copy()
    odd[40, 7] = np.nan
    c, _ = temporal.variance_reference(noise_frame(rng, W, H), None, odd, None, None, None, W, H)
    assert c.reshape(-1, 8)[40, 5] == 3.0


def test_all_static_motion_table_changes_nothing():
    rng = np.random.RandomState(15)
    cam0 = camera()
    objs = scene_inputs("reference", W, H)[0]
    table = temporal.motion_matrices(objs, objs)
    assert np.all(table[:, temporal.M_STATE] == temporal.MOTION_STATIC)
    mom = prev_feat = prev_cam = None
    for k in range(4):
        cam = temporal.orbit_camera(cam0, 1.5 * k)
        feat, rgba = records(cam), noise_frame(rng, W, H)
        plain = temporal.variance_reference(rgba, None, feat, mom, prev_feat, prev_cam, W, H)
        moved = temporal.variance_reference(rgba, None, feat, mom, prev_feat, prev_cam, W, H, motion=table,
                                            n_obj=len(objs))
        assert np.array_equal(plain[0], moved[0]) and np.array_equal(plain[1], moved[1]), k
        mom, prev_feat, prev_cam = plain[0], feat, cam
    assert (mom.reshape(-1, 8)[:, 5] == 1.0).any()


@pytest.mark.parametrize("scene,w,h", (("reference", 64, 48), ("teapot", 28, 20), ("reference", 17, 16),
                                       ("reference", 16, 17), ("reference", 5, 5)))
def test_few_decisions_hang_on_the_last_bits(scene, w, h):
    """The views of tests/test_gpu_variance.py (the 1.5-degree orbit, six frames chained): the pixels the GPU
    comparison may leave out (temporal.variance_undecided) stay within its cap of 1 % of a frame.  The teapot is
    seen at 28 x 20 here: the brute-force comparator is quadratic in pixels x triangles, and the GPU test asserts
    the cap again at its own size."""
    rng = np.random.RandomState(16)
    cam0 = scene_inputs(scene, w, h)[3]
    mom = prev_feat = prev_cam = None
    for k in range(6):
        cam = temporal.orbit_camera(cam0, 1.5 * k)
        feat = records(cam, scene, w, h)
        for radius in (1, 3, 4):
            res = temporal.variance_reference(noise_frame(rng, w, h), None, feat, mom, prev_feat, prev_cam, w, h,
                                              dict(radius=radius), details=True)
            left_out = int(temporal.variance_undecided(res[2], w, h, dict(radius=radius)).sum())
            print("%s %dx%d frame %d radius %d: %d pixels undecided" % (scene, w, h, k, radius, left_out))
            assert left_out <= 0.01 * w * h
        mom, prev_feat, prev_cam = res[0], feat, cam
