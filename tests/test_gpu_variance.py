"""The device kernel of variance estimation (ptmi_variance_estimate) against its numpy statement
(ptmi/temporal.py variance_reference) on chained real renders, on the smallest shapes, and its parameters.

Frames: the reference scene and the teapot at 64 x 48, six frames of 1 spp and of 4 spp with a different seed
stream per frame on a 1.5-degree-per-frame orbit, and the reference scene with a fixed camera whose larger ball
(object 7) moves by 0.05 in x per frame (tests/test_gpu_motion_sequence.py's step) through the motion table.  Each
frame's call reads the device's own moment record of the frame before, and numpy restates that one call from the
same inputs, so a pixel left out in one frame does not spread.  The window's radius changes from frame to frame
(3, 1, 4, 2, 3, 4): the moments do not depend on it.

Tolerance: none.  Every operation of the kernel is an IEEE FP64 add, multiply, divide, square root or comparison
in the order the numpy statement gives, and the record and out_se are compared bit for bit -- outside the pixels one
of whose discontinuous decisions hangs on the last bits (temporal.variance_undecided), at most 1 % of a frame."""
import numpy as np
import pytest

from ptmi import api, geom, temporal
from tests.scene_inputs import scene_inputs
from tests.test_gpu_rectify import _outputs, _up
from tests.test_temporal_reference import records

pytestmark = pytest.mark.gpu
W, H, FRAMES, STEP, BALL, SHIFT = 64, 48, 6, 1.5, 7, 0.05
RADII = (3, 1, 4, 2, 3, 4)
CASES = (("reference", 1, False), ("reference", 4, False), ("teapot", 1, False), ("teapot", 4, False),
         ("reference", 4, True))
_cache = {}


def _frames(scene, spp, moving):
    """Per frame (camera, image, se, feat, objects) as numpy arrays: rendered once per case."""
    import torch
    key = (scene, spp, moving)
    if key not in _cache:
        objs, tris, grps, cam = scene_inputs(scene, W, H)
        cams = [cam if moving else temporal.orbit_camera(cam, k * STEP) for k in range(FRAMES)]
        objects = [temporal.move_object(objs, BALL, geom.translate(SHIFT * k, 0.0, 0.0)) for k in range(FRAMES)] \
            if moving else None
        sc = api.Scene(0, objs, tris, grps, cam)
        out = []
        seq = temporal.render_sequence(sc, cams, spp, 900, temporal=False, chunks=2 if tris.size else 0, objects=objects)
        for k, (c, f) in enumerate(zip(cams, seq)):
            torch.cuda.synchronize()
            out.append((c, f["image"].cpu().numpy(), f["se"].cpu().numpy(), f["feat"].cpu().numpy(),
                        objects[k] if moving else None))
        sc.close()
        _cache[key] = out
    return _cache[key]


def _estimate(image, se, feat, prev, w, h, params=None, motion=None, n_obj=0):
    """(mom, out_se) of one device call on canary-guarded outputs; prev: (mom, feat, camera) or None."""
    d = [_up(image), _up(se) if se is not None else None, _up(feat)] + ([_up(prev[0]), _up(prev[1])] if prev else [])
    m = _up(motion) if motion is not None else None

    def call(b):
        api.variance_estimate(d[0].data_ptr(), d[1].data_ptr() if se is not None else 0, d[2].data_ptr(),
                              d[3].data_ptr() if prev else 0, d[4].data_ptr() if prev else 0, prev[2] if prev else None,
                              w, h, b[0].data_ptr(), b[1].data_ptr(), motion_ptr=m.data_ptr() if m is not None else 0,
                              n_obj=n_obj, params=params)
    return _outputs((8, 1), w * h, call, (True, True))


def _same_bits(dev, ref, keep, label):
    """The record and out_se bit for bit over the pixels `keep`; the differences are printed first."""
    (md, sd), (mr, sr) = [(a.reshape(-1, 8), b) for a, b in (dev, ref)]
    k = keep.reshape(-1)
    with np.errstate(all="ignore"):
        diff = np.nan_to_num(np.abs(md[k] - mr[k]), nan=0.0, posinf=0.0)
        dse = np.nan_to_num(np.abs(sd[k] - sr[k]), nan=0.0, posinf=0.0)
    src = md[:, 5]
    print("%s: %d of %d pixels left out; sources none/temporal/spatial/fallback %d/%d/%d/%d; max |device - numpy| "
          "per slot %s, out_se %.3e" % (label, int((~k).sum()), k.size, *[(src == v).sum() for v in (0, 1, 2, 3)],
                                        " ".join("%.1e" % v for v in diff.max(0)) if k.any() else "-",
                                        dse.max() if k.any() else 0.0))
    assert (~k).sum() <= 0.01 * k.size
    assert np.array_equal(md[k], mr[k], equal_nan=True), label
    assert np.array_equal(sd[k], sr[k], equal_nan=True), label
    assert np.all(md[:, 7] == 0.0) and np.isin(src, (0.0, 1.0, 2.0, 3.0)).all()


@pytest.mark.parametrize("scene,spp,moving", CASES)
def test_device_matches_numpy_on_chained_renders(scene, spp, moving):
    frames = _frames(scene, spp, moving)
    prev, seen = None, set()
    for k, (cam, image, se, feat, objs) in enumerate(frames):
        motion, n_obj = None, 0
        if moving and k:
            motion, n_obj = temporal.motion_matrices(frames[k - 1][4], objs), len(objs)
        params = dict(radius=RADII[k])
        dev = _estimate(image, se, feat, prev, W, H, params, motion, n_obj)
        mom, out_se, info = temporal.variance_reference(image, se, feat, prev[0] if prev else None,
                                                        prev[1] if prev else None, prev[2] if prev else None, W, H,
                                                        params, details=True, motion=motion, n_obj=n_obj)
        keep = ~temporal.variance_undecided(info, W, H, params)
        _same_bits(dev, (mom, out_se), keep, "%s %d spp%s frame %d r=%d" % (scene, spp, " moving" if moving else "", k,
                                                                           RADII[k]))
        seen |= set(np.unique(dev[0].reshape(-1, 8)[:, 5]))
        prev = (dev[0], feat, cam)
    m = dev[0].reshape(-1, 8)
    hit = feat.reshape(-1, 12)[:, 7] >= 0
    assert {1.0, 2.0} <= seen, "both estimates were taken along the chain"
    assert (m[hit, 4] > 4.0).mean() > 0.7 and (m[hit, 5] == 1.0).mean() > 0.7, "the moment history grew"
    if moving:
        ball = feat.reshape(-1, 12)[:, 7] == BALL
        assert m[ball, 4].mean() > 3.0, "and the ball's pixels followed it"
    if spp == 1:
        assert np.isinf(se).all() and np.isfinite(dev[1]).all(), "1 spp: the rendered map is +inf, the estimate is not"


@pytest.mark.parametrize("w,h", ((17, 16), (16, 17), (5, 5), (1, 1)))
@pytest.mark.parametrize("radius", (1, 4))
def test_smallest_shapes(w, h, radius):
    """A partial block next to a whole one in x and in y (the halo crosses the block's edge), a window larger than
    the image, and one pixel (the fallback).  Records of the reference scene by the brute-force comparator,
    synthetic colours, three chained frames on the orbit; min_temporal = 2, so that both estimates are taken."""
    rng = np.random.RandomState(100 * w + h)
    cam0 = scene_inputs("reference", w, h)[3]
    params = dict(radius=radius, min_temporal=2)
    prev = None
    for k in range(3):
        cam = temporal.orbit_camera(cam0, k * STEP)
        feat = records(cam, "reference", w, h).reshape(-1)
        image = np.ones((w * h, 4))
        image[:, :3] = 0.5 + 0.25 * rng.rand(w * h, 3)
        se = 0.05 + rng.rand(w * h) if k != 1 else None
        dev = _estimate(image, se, feat, prev, w, h, params)
        mom, out_se, info = temporal.variance_reference(image, se, feat, prev[0] if prev else None,
                                                        prev[1] if prev else None, prev[2] if prev else None, w, h,
                                                        params, details=True)
        keep = ~temporal.variance_undecided(info, w, h, params)
        _same_bits(dev, (mom, out_se), keep, "%dx%d r=%d frame %d" % (w, h, radius, k))
        if k == 0 and (w, h) == (1, 1):
            assert dev[0][5] == 3.0 and dev[0][6] == se[0] * se[0], "one pixel: the fallback"
        prev = (dev[0], feat, cam)


def test_canaries_parameters_and_the_optional_map():
    frames = _frames("reference", 4, False)
    prev = None
    for cam, image, se, feat, _ in frames[:2]:
        prev = (_estimate(image, se, feat, prev, W, H)[0], feat, cam)
    cam, image, se, feat, _ = frames[2]
    base = _estimate(image, se, feat, prev, W, H)
    again = _estimate(image, se, feat, prev, W, H)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(base, again)), "two identical calls differ"
    explicit = _estimate(image, se, feat, prev, W, H, api.VarianceParams(32, 4, 3, 9, 0, 0.9, 0.02, 0.05, 0.9))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(base, explicit))
    b = base[0].reshape(-1, 8)
    assert (b[:, 5] == 2.0).mean() > 0.8, "the third frame's history is shorter than min_temporal: the window"
    for change in (dict(min_temporal=2), dict(radius=1), dict(window_normal_cos=0.999), dict(min_count=40)):
        other = _estimate(image, se, feat, prev, W, H, change)
        mom, out_se, info = temporal.variance_reference(image, se, feat, prev[0], prev[1], prev[2], W, H, change,
                                                        details=True)
        o = other[0].reshape(-1, 8)
        assert not np.array_equal(other[1], base[1], equal_nan=True), "%r reaches the kernel" % (change,)
        _same_bits(other, (mom, out_se), ~temporal.variance_undecided(info, W, H, change), "parameters %r" % (change,))
        if "min_temporal" in change:
            assert (o[:, 5] == 1.0).mean() > 0.7
    short = _estimate(image, se, feat, prev, W, H, dict(max_history=2))[0].reshape(-1, 8)
    assert short[:, 4].max() == 2.0 and b[:, 4].max() > 2.5, "max_history reaches the kernel"
    # se_dev = NULL: another fallback, and nothing else
    none = _estimate(image, None, feat, prev, W, H, dict(min_count=40))
    given = _estimate(image, se, feat, prev, W, H, dict(min_count=40))
    n, g = none[0].reshape(-1, 8), given[0].reshape(-1, 8)
    fb = g[:, 5] == 3.0
    assert fb.any() and (~fb).any() and np.array_equal(n[:, :6], g[:, :6], equal_nan=True)
    assert np.array_equal(n[~fb], g[~fb], equal_nan=True) and np.array_equal(none[1][~fb], given[1][~fb], equal_nan=True)
    c = image.reshape(-1, 4)[:, :3]
    s = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    assert np.array_equal(n[fb, 6], s[fb]) and np.array_equal(g[fb, 6], (se * se)[fb])
    assert (n[fb, 6] != g[fb, 6]).any()
    # a pixel that is not finite: N = 0, the input's se (or +inf), and no tap for its neighbours' windows
    image2 = image.copy()
    image2[4 * 1000 + 1] = np.nan
    y, x = divmod(1000, W)
    far = np.ones((H, W), dtype=bool)
    far[y - 3:y + 4, x - 3:x + 4] = False
    for se_arg in (se, None):
        bad = _estimate(image2, se_arg, feat, prev, W, H)
        rec = bad[0].reshape(-1, 8)[1000]
        assert np.isnan(rec[1]) and np.isnan(rec[3]) and np.all(rec[4:] == 0.0)
        assert bad[1][1000] == (se[1000] if se_arg is not None else np.inf)
        if se_arg is not None:
            assert np.array_equal(bad[0].reshape(H, W, 8)[far], base[0].reshape(H, W, 8)[far], equal_nan=True)
            near = ~far.reshape(-1)
            near[1000] = False
            assert (bad[0].reshape(-1, 8)[near, 6] != b[near, 6]).any(), "its neighbours' windows lost a tap"
            assert np.isfinite(bad[0].reshape(-1, 8)[near]).all()
