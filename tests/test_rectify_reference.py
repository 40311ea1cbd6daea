"""The numpy statements of history rectification (ptmi/temporal.py gather_reference, rectify_reference) on
the CPU: synthetic frames whose outcome is known without a device.

gather_reference shares reproject_reference's body, so with the test switched off (min_count above the
window's size) gather + rectify must reproduce reproject_reference bit for bit; the other cases pin down the
window, the test and the resets one at a time."""
import numpy as np
import pytest

from ptmi import temporal
from tests.scene_inputs import scene_inputs

W, H = 20, 12
OFF = dict(min_count=1000)  # more than (2 * 4 + 1)^2 taps: no window is ever tested


def _frame(colour, se, ids=0.0, w=W, h=H):
    rgba = np.ones((h, w, 4))
    rgba[..., :3] = colour
    feat = np.zeros((h, w, temporal.FEATURE_DOUBLES))
    feat[..., temporal.F_ID] = ids
    return rgba, np.full((h, w), float(se)), feat


def _gathered(colour, var, n, w=W, h=H):
    g = np.zeros((h, w, temporal.HISTORY_DOUBLES))
    g[..., :3], g[..., 3], g[..., 4] = colour, var, n
    return g


def _blend(c, v, hc, hv, hn, max_history=32.0):
    """reproject_reference's blend, in its operations and order."""
    np1 = hn + 1.0
    n = np.where(np1 < max_history, np1, max_history)
    a = 1.0 / n
    b = 1.0 - a
    return hc + a[..., None] * (c - hc), (a * a) * v + (b * b) * hv, n


def test_constant_colour_and_history_blend_exactly():
    colour = np.array([0.3, 0.7, 0.1])
    rgba, se, feat = _frame(colour, 0.05)
    g = _gathered(colour, 0.001, 5.0)
    for r in (1, 3, 4):
        hist, out, out_se = temporal.rectify_reference(rgba, se, feat, g, W, H, dict(radius=r))
        hist = hist.reshape(H, W, 8)
        c, v, n = _blend(rgba[..., :3], se * se, g[..., :3], g[..., 3], g[..., 4])
        assert np.array_equal(hist[..., :3], c) and np.array_equal(hist[..., :3], np.broadcast_to(colour, (H, W, 3)))
        assert np.array_equal(hist[..., 3], v) and np.array_equal(hist[..., 4], n) and np.all(n == 6.0)
        assert np.all(hist[..., 5] == 1.0) and np.all(hist[..., 6:] == 0.0)
        assert np.array_equal(out.reshape(H, W, 4)[..., :3], c) and np.all(out[3::4] == 1.0)
        assert np.array_equal(out_se.reshape(H, W), np.sqrt(v))


_records_cache = {}


def _records(objs, cam, w, h):
    """feat[H*W, 12] of the reference scene with these objects through `cam` (the brute-force comparator)."""
    from tests import features_ref
    key = (np.ascontiguousarray(objs).tobytes(), np.asarray(cam).tobytes())
    if key not in _records_cache:
        _, tris, grps, _ = scene_inputs("reference", w, h)
        ref = features_ref.closest_hits(objs, tris, grps, cam, w, h)
        f = np.zeros((w * h, temporal.FEATURE_DOUBLES))
        f[:, 0:3], f[:, 3], f[:, 4:7], f[:, 7], f[:, 8:11] = ref["pos"], ref["t"], ref["normal"], ref["id"], ref["albedo"]
        _records_cache[key] = f
    return _records_cache[key]


@pytest.mark.parametrize("with_motion", (False, True))
def test_switched_off_equals_reproject_reference(with_motion):
    """Random finite colours, errors and histories on the reference scene's real records, the previous frame
    seen from a camera 2 degrees off (and, with the motion, the larger ball 0.05 further left)."""
    from ptmi import geom
    w, h = 28, 20
    rng = np.random.default_rng(5)
    objs, _, _, cam = scene_inputs("reference", w, h)
    prev_cam = temporal.orbit_camera(cam, -2.0)
    cur_objs = temporal.move_object(objs, 7, geom.translate(0.05, 0.0, 0.0)) if with_motion else objs
    kw = dict(motion=temporal.motion_matrices(objs, cur_objs), n_obj=len(objs)) if with_motion else {}
    f, pf = _records(cur_objs, cam, w, h), _records(objs, prev_cam, w, h)
    rgba = np.ones((w * h, 4))
    rgba[:, :3] = rng.uniform(0.0, 2.0, (w * h, 3))
    se = rng.uniform(0.01, 0.5, w * h)
    prev = np.zeros((w * h, 8))
    prev[:, :3], prev[:, 3], prev[:, 4] = rng.uniform(0.0, 2.0, (w * h, 3)), rng.uniform(1e-4, 0.1, w * h), \
        rng.integers(1, 9, w * h).astype(np.float64)
    want = temporal.reproject_reference(rgba, se, f, prev, pf, prev_cam, w, h, **kw)
    g = temporal.gather_reference(rgba, se, f, prev, pf, prev_cam, w, h, **kw)
    got = temporal.rectify_reference(rgba, se, f, g, w, h, OFF)
    assert (want[0].reshape(-1, 8)[:, 4] > 1.0).sum() > 0.3 * w * h, "many pixels blend a history"
    assert (g.reshape(-1, 8)[:, 4] == 0.0).any(), "and some find none"
    assert np.array_equal(got[0].reshape(-1, 8)[:, :5], want[0].reshape(-1, 8)[:, :5])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.all(got[0].reshape(-1, 8)[:, 5] == 1.0) and np.all(g.reshape(-1, 8)[:, 5:] == 0.0)
    # with the test on, random colours against random histories are rectified somewhere
    on = temporal.rectify_reference(rgba, se, f, g, w, h, dict(gamma=0.5))[0].reshape(-1, 8)
    assert (on[:, 5] < 1.0).any() and not np.array_equal(on[:, :5], want[0].reshape(-1, 8)[:, :5])
    # the first frame: no history anywhere
    want0 = temporal.reproject_reference(rgba, se, f, None, None, None, w, h)
    g0 = temporal.gather_reference(rgba, se, f, None, None, None, w, h)
    assert np.all(g0.reshape(-1, 8)[:, 4] == 0.0)
    got0 = temporal.rectify_reference(rgba, se, f, g0, w, h)
    assert np.array_equal(got0[0].reshape(-1, 8)[:, :5], want0[0].reshape(-1, 8)[:, :5])


def test_noise_free_step_forgets_the_history():
    rgba, se, feat = _frame(0.2, 0.0)
    g = _gathered(1.0, 0.0, 7.0)
    hist, out, out_se = temporal.rectify_reference(rgba, se, feat, g, W, H)
    hist = hist.reshape(H, W, 8)
    assert np.all(hist[..., 5] == 0.0) and np.all(hist[..., 4] == 1.0)
    assert np.array_equal(hist[..., :3], rgba[..., :3]) and np.all(hist[..., 3] == 0.0)


def test_objects_do_not_see_each_other():
    ids = np.zeros((H, W))
    ids[:, W // 2:] = 1.0
    rgba, se, feat = _frame(0.5, 0.01, ids)
    hcol = np.where(ids[..., None] == 0.0, 0.5, 0.9) * np.ones((H, W, 3))  # left: history right; right: off by 0.4
    g = _gathered(hcol, 1e-4, 8.0)
    hist, _, _, info = temporal.rectify_reference(rgba, se, feat, g, W, H, details=True)
    hist = hist.reshape(H, W, 8)
    left, right = ids == 0.0, ids == 1.0
    assert np.all(hist[left, 5] == 1.0), "up to the boundary column the left half is not rectified"
    assert np.all(hist[right, 5] < 0.2), "and the right half is, from its first column on"
    assert np.all(hist[left, 4] == 9.0) and np.all(hist[right, 4] < 3.0)
    assert info["m"][H // 2, W // 2 - 1] == 7 * 4 and info["m"][H // 2, W // 2] == 7 * 4
    # the same frame with one id everywhere: the boundary columns now see the other side
    one = temporal.rectify_reference(rgba, se, _frame(0.5, 0.01)[2], g, W, H)[0].reshape(H, W, 8)
    assert np.all(one[:, W // 2 - 1, 5] < 1.0)


def test_unusable_taps_are_skipped():
    rgba, se, feat = _frame(0.5, 0.01)
    g = _gathered(0.5, 1e-4, 8.0)
    y, x = 6, 10
    rgba[y, x - 1, 1] = np.nan        # a tap whose colour is not finite
    se[y - 1, x] = np.inf             # ... whose se is not
    g[y + 1, x, 4] = 0.0              # ... without history
    g[y + 1, x, :3] = 1e6             # (its record is never read)
    feat[y, x + 1, temporal.F_ID] = np.nan  # a NaN id matches nothing
    hist, _, _, info = temporal.rectify_reference(rgba, se, feat, g, W, H, dict(radius=1), details=True)
    hist = hist.reshape(H, W, 8)
    assert info["m"][y, x] == 9 - 4
    assert hist[y, x, 5] == 1.0 and hist[y, x, 4] == 9.0 and np.all(hist[y, x, :3] == 0.5)
    # the resets: not finite -> N = 0 with the input's bits; no history -> N = 1; a NaN id has no window (m = 0)
    assert hist[y, x - 1, 4] == 0.0 and np.isnan(hist[y, x - 1, 1]) and hist[y, x - 1, 5] == 1.0
    assert hist[y - 1, x, 4] == 0.0 and hist[y - 1, x, 3] == np.inf
    assert hist[y + 1, x, 4] == 1.0 and np.all(hist[y + 1, x, :3] == 0.5) and hist[y + 1, x, 3] == 0.01 * 0.01
    assert info["m"][y, x + 1] == 0 and hist[y, x + 1, 5] == 1.0 and hist[y, x + 1, 4] == 9.0
    assert np.isfinite(np.delete(hist.reshape(-1, 8), [(y * W + x - 1), (y - 1) * W + x], axis=0)).all()


def test_corner_window_and_min_count():
    rgba, se, feat = _frame(0.2, 0.0)
    g = _gathered(1.0, 0.0, 7.0)
    info = temporal.rectify_reference(rgba, se, feat, g, W, H, dict(radius=3), details=True)[3]
    assert info["m"][0, 0] == 16 and info["m"][H - 1, W - 1] == 16 and info["m"][0, W - 1] == 16
    assert info["m"][5, 10] == 49 and info["m"][0, 10] == 28
    for min_count, rectified in ((16, True), (17, False)):
        hist = temporal.rectify_reference(rgba, se, feat, g, W, H, dict(radius=3, min_count=min_count))[0].reshape(H, W, 8)
        assert (hist[0, 0, 5] == 0.0) == rectified and (hist[0, 0, 4] == (1.0 if rectified else 8.0))
        assert hist[5, 10, 5] == 0.0


def test_a_tie_does_not_rectify():
    """d2 == T2 exactly.  Colour 0 and history (0.5, 0, 0) over the 9 taps of an interior pixel at radius 1
    give d = (4.5 / 9, 0, 0) and d2 = 0.25; se = 1.5 and hv = 0 give V = (9 * 2.25 + 0) / 81 = 0.25, and
    gamma = 1 makes T2 = 0.25: every step is exact in binary."""
    rgba, se, feat = _frame(0.0, 1.5)
    g = _gathered(np.array([0.5, 0.0, 0.0]), 0.0, 4.0)
    hist, _, _, info = temporal.rectify_reference(rgba, se, feat, g, W, H, dict(radius=1, gamma=1.0), details=True)
    hist = hist.reshape(H, W, 8)
    assert info["d2"][5, 5] == 0.25 and info["T2"][5, 5] == 0.25
    assert hist[5, 5, 5] == 1.0 and hist[5, 5, 4] == 5.0
    # one ulp less tolerance: rectified, rho just below 1
    below = temporal.rectify_reference(rgba, se, feat, g, W, H, dict(radius=1, gamma=np.nextafter(1.0, 0.0)))[0]
    assert below.reshape(H, W, 8)[5, 5, 5] < 1.0
    # a NaN tolerance (inf - inf variances) leaves the history as found
    g2 = g.copy()
    g2[..., 3] = np.inf
    nan = temporal.rectify_reference(rgba, se, feat, g2, W, H, dict(radius=1, gamma=0.0))[0].reshape(H, W, 8)
    assert nan[5, 5, 5] == 1.0


def test_parameters_are_checked():
    assert temporal.rectify_params_dict(None) == temporal.RECTIFY_DEFAULTS == \
        dict(radius=3, min_count=9, gamma=3.0, max_history=32, flags=0)
    assert temporal.rectify_params_dict(True) == temporal.RECTIFY_DEFAULTS
    for bad in (dict(radius=0), dict(radius=5), dict(gamma=-1.0), dict(gamma=float("nan")), dict(max_history=0),
                dict(max_history=65537), dict(flags=1)):
        with pytest.raises(ValueError):
            temporal.rectify_params_dict(bad)
