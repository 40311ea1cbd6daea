"""The device kernels of history rectification (ptmi_history_gather, ptmi_rectify) against their numpy
statements (ptmi/temporal.py gather_reference, rectify_reference) on real renders, and against the calls
they take the place of.

Frames: the reference scene at 64 x 48 and the teapot at 48 x 36, 8 spp per frame, a different seed stream per
frame, the camera orbiting by 1.5 degrees per frame; and the reference scene at 20 x 12, where the 16 x 16
blocks are partial in both directions and a block's halo crosses the image edge on all four sides.  Four
frames per case: ptmi_reproject chains the first three into a real history (fractional N, non-trivial
variances), and the fourth is the frame under test.

Tolerance: tests/test_gpu_reproject.py's rule.  Every operation of both kernels is an IEEE FP64 add,
multiply, divide or square root in the order the numpy statements give; |device - numpy| <= 1e-9 x the
frame's largest channel value for colour and variance, 1e-9 x max_history for N and 1e-9 for rho, outside
the pixels one of whose discontinuous decisions in the lookup hangs on the last bits (temporal.undecided),
at most 1 % of a frame.  Rectification has no discontinuous decision of its own -- m is an integer and rho
is continuous at d2 = T2 -- but its window reads the neighbours' gathered records, so for ptmi_rectify on
the device's own gathered record the pixels within `radius` of an undecided one are left out with it, under
the same 1 % cap; given numpy's gathered record nothing is left out."""
import numpy as np
import pytest

from ptmi import api, geom, temporal
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu
CASES = (("reference", 64, 48), ("teapot", 48, 36), ("reference", 20, 12))
SPP, FRAMES, STEP, CANARY, PAD, BALL = 8, 4, 1.5, -12345.0, 64, 7
RADII = (1, 3, 4)
OFF = dict(min_count=1000)
_cache = {}


def _up(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.float64, device="cuda")


def _frames(scene, w, h, moving=False):
    """Per frame (camera, image, se, feat, objects) as numpy arrays: rendered once per case.  moving: the
    camera stands still and the larger ball moves by 0.05 in x per frame."""
    import torch
    key = (scene, w, h, moving)
    if key not in _cache:
        objs, tris, grps, cam = scene_inputs(scene, w, h)
        cams = [cam if moving else temporal.orbit_camera(cam, k * STEP) for k in range(FRAMES)]
        objects = [temporal.move_object(objs, BALL, geom.translate(0.05 * k, 0.0, 0.0)) for k in range(FRAMES)] \
            if moving else None
        sc = api.Scene(0, objs, tris, grps, cam)
        out = []
        seq = temporal.render_sequence(sc, cams, SPP, 700, temporal=False, chunks=2 if tris.size else 0, objects=objects)
        for k, (c, f) in enumerate(zip(cams, seq)):
            torch.cuda.synchronize()
            out.append((c, f["image"].cpu().numpy(), f["se"].cpu().numpy(), f["feat"].cpu().numpy(),
                        objects[k] if moving else None))
        sc.close()
        _cache[key] = out
    return _cache[key]


def _outputs(sizes, n, call, used):
    """Run `call(buffers)` on canary-filled buffers of n * size + PAD doubles; check the canaries."""
    import torch
    bufs = [torch.full((n * k + PAD,), CANARY, dtype=torch.float64, device="cuda") for k in sizes]
    call(bufs)
    torch.cuda.synchronize()
    res = [b.cpu().numpy() for b in bufs]
    for b, k, u in zip(res, sizes, used):
        assert np.all(b[n * k:] == CANARY), "the canary behind an output was overwritten"
        if not u:
            assert np.all(b == CANARY), "an output that was not asked for was written"
    return [b[:n * k] if u else None for b, k, u in zip(res, sizes, used)]


def _reproject(image, se, feat, prev, w, h, motion=None, n_obj=0, params=None):
    d = [_up(image), _up(se), _up(feat)] + ([_up(prev[0]), _up(prev[1])] if prev else [])
    m = _up(motion) if motion is not None else None

    def call(b):
        args = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr() if prev else 0,
                d[4].data_ptr() if prev else 0, prev[2] if prev else None, w, h, b[0].data_ptr())
        kw = dict(out_rgba_ptr=b[1].data_ptr(), out_se_ptr=b[2].data_ptr(), params=params)
        if m is not None:
            api.reproject_motion(*args, m.data_ptr(), n_obj, **kw)
        else:
            api.reproject(*args, **kw)
    return _outputs((8, 4, 1), w * h, call, (True, True, True))


def _gather(image, se, feat, prev, w, h, motion=None, n_obj=0, params=None):
    d = [_up(image), _up(se), _up(feat)] + ([_up(prev[0]), _up(prev[1])] if prev else [])
    m = _up(motion) if motion is not None else None

    def call(b):
        api.history_gather(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr() if prev else 0,
                           d[4].data_ptr() if prev else 0, prev[2] if prev else None, w, h, b[0].data_ptr(),
                           motion_ptr=m.data_ptr() if m is not None else 0, n_obj=n_obj, params=params)
    return _outputs((8,), w * h, call, (True,))[0]


def _rectify(image, se, feat, gathered, w, h, params=None, want_rgba=True, want_se=True):
    d = [_up(image), _up(se), _up(feat), _up(gathered)]

    def call(b):
        api.rectify(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), w, h, b[0].data_ptr(),
                    out_rgba_ptr=b[1].data_ptr() if want_rgba else 0, out_se_ptr=b[2].data_ptr() if want_se else 0,
                    params=params)
    return _outputs((8, 4, 1), w * h, call, (True, want_rgba, want_se))


def _history(frames, w, h, upto):
    """ptmi_reproject chained over frames[:upto]: (hist, feat, camera) of the last of them."""
    prev = None
    for cam, image, se, feat, _ in frames[:upto]:
        prev = (_reproject(image, se, feat, prev, w, h)[0], feat, cam)
    return prev


def _dilate(mask, r):
    out = mask.copy()
    h, w = mask.shape
    for y, x in zip(*np.nonzero(mask)):
        out[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return out


def _close(dev, ref, keep, max_history, label, rho):
    hd, hr = dev.reshape(-1, 8), ref.reshape(-1, 8)
    fin = np.isfinite(hr[:, :4]).all(1)
    assert np.array_equal(hd[~fin], hr[~fin], equal_nan=True)  # pixels that are not finite: the input's bits
    m = keep.reshape(-1) & fin
    scale = np.abs(hr[fin, :3]).max()
    d_c = np.abs(hd[m, :3] - hr[m, :3]).max() / scale
    d_v = np.abs(hd[m, 3] - hr[m, 3]).max() / scale
    d_n = np.abs(hd[m, 4] - hr[m, 4]).max() / max_history
    d_r = np.abs(hd[m, 5] - hr[m, 5]).max()
    print("%s: %d of %d pixels left out; max |device - numpy|: colour %.3e, variance %.3e of the largest channel, "
          "N %.3e of max_history, [5] %.3e; bit-equal %s" % (label, int((~keep).sum()), keep.size, d_c, d_v, d_n, d_r,
                                                            np.array_equal(hd, hr, equal_nan=True)))
    assert (~keep).sum() <= 0.01 * keep.size
    assert d_c <= 1e-9 and d_v <= 1e-9 and d_n <= 1e-9 and d_r <= 1e-9
    assert np.all(hd[:, 6:] == 0.0) and (rho or np.all(hd[:, 5] == 0.0))


@pytest.mark.parametrize("scene,w,h", CASES)
def test_device_matches_numpy(scene, w, h):
    frames = _frames(scene, w, h)
    prev = _history(frames, w, h, FRAMES - 1)
    cam, image, se, feat, _ = frames[-1]
    g_dev = _gather(image, se, feat, prev, w, h)
    again = _gather(image, se, feat, prev, w, h)
    assert np.array_equal(g_dev, again, equal_nan=True), "two identical calls differ"
    g_ref, info = temporal.gather_reference(image, se, feat, prev[0], prev[1], prev[2], w, h, details=True)
    und = temporal.undecided(info, w, h)
    label = "%s %dx%d" % (scene, w, h)
    _close(g_dev, g_ref, ~und, 32.0, label + " gather", rho=False)
    n = g_dev.reshape(-1, 8)[:, 4]
    print("%s: %d of %d pixels found a history, N up to %g" % (label, int((n > 0.0).sum()), w * h, n.max()))
    assert (n > 1.0).sum() > 0.5 * w * h, "most pixels find a history of more than one frame"
    for r in RADII:
        params = dict(radius=r, gamma=1.0)  # (a tolerance at which a good part of the frame is rectified)
        ref = temporal.rectify_reference(image, se, feat, g_ref, w, h, params)
        dev = _rectify(image, se, feat, g_dev, w, h, params)
        _close(dev[0], ref[0], ~_dilate(und, r), 32.0, "%s rectify r=%d" % (label, r), rho=True)
        rho = dev[0].reshape(-1, 8)[:, 5]
        assert (rho < 1.0).any() and (rho == 1.0).any() and np.all((rho >= 0.0) & (rho <= 1.0))
        # the optional outputs are (c', 1) and sqrt(var') of the history, bit for bit
        hd = dev[0].reshape(-1, 8)
        assert np.array_equal(dev[1].reshape(-1, 4)[:, :3], hd[:, :3], equal_nan=True) and np.all(dev[1][3::4] == 1.0)
        assert np.array_equal(dev[2], np.sqrt(hd[:, 3]), equal_nan=True)
        # given numpy's gathered record: nothing left out
        same = _rectify(image, se, feat, g_ref, w, h, params)
        _close(same[0], ref[0], np.ones((h, w), dtype=bool), 32.0, "%s rectify r=%d on numpy's record" % (label, r),
               rho=True)
        default = _rectify(image, se, feat, g_ref, w, h, dict(radius=r))
        _close(default[0], temporal.rectify_reference(image, se, feat, g_ref, w, h, dict(radius=r))[0],
               np.ones((h, w), dtype=bool), 32.0, "%s rectify r=%d gamma 3" % (label, r), rho=True)


@pytest.mark.parametrize("moving", (False, True))
def test_switched_off_is_the_reprojection_bit_for_bit(moving):
    """min_count = 1000: gather + rectify against ptmi_reproject / ptmi_reproject_motion over four chained frames,
    each path feeding on its own history."""
    scene, w, h = CASES[0]
    frames = _frames(scene, w, h, moving)
    prev_a = prev_b = None
    for k, (cam, image, se, feat, objs) in enumerate(frames):
        motion, n_obj = None, 0
        if moving and k:
            motion, n_obj = temporal.motion_matrices(frames[k - 1][4], objs), len(objs)
        a = _reproject(image, se, feat, prev_a, w, h, motion, n_obj)
        g = _gather(image, se, feat, prev_b, w, h, motion, n_obj)
        b = _rectify(image, se, feat, g, w, h, OFF)
        assert np.array_equal(b[0].reshape(-1, 8)[:, :5], a[0].reshape(-1, 8)[:, :5], equal_nan=True), k
        assert np.array_equal(b[1], a[1], equal_nan=True) and np.array_equal(b[2], a[2], equal_nan=True), k
        assert np.all(b[0].reshape(-1, 8)[:, 5] == 1.0) and np.all(b[0].reshape(-1, 8)[:, 6:] == 0.0)
        prev_a, prev_b = (a[0], feat, cam), (b[0], feat, cam)  # (b's [5] = rho is read by no lookup)
    n = a[0].reshape(-1, 8)[:, 4]
    assert (n > 3.0).sum() > 0.5 * w * h, "the fourth frame read three frames of history"
    if moving:
        ball = feat.reshape(-1, 12)[:, 7] == BALL
        assert n[ball].mean() > 2.0, "and the ball's pixels followed it"


def test_optional_outputs_and_defaults():
    scene, w, h = CASES[2]
    frames = _frames(scene, w, h)
    prev = _history(frames, w, h, FRAMES - 1)
    cam, image, se, feat, _ = frames[-1]
    g = _gather(image, se, feat, prev, w, h)
    assert np.array_equal(g, _gather(image, se, feat, prev, w, h, params=api.ReprojectParams(32, 0, 0.9, 0.02, 0.05)),
                          equal_nan=True)
    full = _rectify(image, se, feat, g, w, h)
    for want_rgba, want_se in ((False, False), (True, False), (False, True)):
        part = _rectify(image, se, feat, g, w, h, want_rgba=want_rgba, want_se=want_se)
        assert np.array_equal(part[0], full[0], equal_nan=True)
        assert part[1] is None or np.array_equal(part[1], full[1], equal_nan=True)
        assert part[2] is None or np.array_equal(part[2], full[2], equal_nan=True)
    explicit = _rectify(image, se, feat, g, w, h, api.RectifyParams(3, 9, 3.0, 32, 0))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(explicit, full))
    other = _rectify(image, se, feat, g, w, h, dict(max_history=2))[0].reshape(-1, 8)
    assert other[:, 4].max() == 2.0, "max_history reaches the kernel"
    # a first frame needs no previous records or camera: every pixel N = 0, then N = 1 (0 where not finite)
    image2, se2 = image.copy(), se.copy()
    image2[4 * 7 + 1], se2[11] = np.nan, np.inf
    g0 = _gather(image2, se2, feat, None, w, h).reshape(-1, 8)
    assert np.all(g0[:, 4:] == 0.0) and np.isnan(g0[7, 1]) and g0[11, 3] == np.inf
    first = _rectify(image2, se2, feat, g0, w, h)[0].reshape(-1, 8)
    want = _reproject(image2, se2, feat, None, w, h)[0].reshape(-1, 8)
    assert np.array_equal(first[:, :5], want[:, :5], equal_nan=True) and first[7, 4] == 0.0 and first[11, 4] == 0.0
    # ... and such pixels are no history and no tap for the next frame
    nxt_g = _gather(image, se, feat, (first.reshape(-1), feat, cam), w, h)
    nxt = _rectify(image, se, feat, nxt_g, w, h)
    ref_g = temporal.gather_reference(image, se, feat, first.reshape(-1), feat, cam, w, h)
    ref = temporal.rectify_reference(image, se, feat, ref_g, w, h)
    _close(nxt[0], ref[0], np.ones((h, w), dtype=bool), 32.0, "after a frame with non-finite pixels", rho=True)
    assert np.isfinite(nxt[0]).all()
    mixed = _rectify(image2, se2, feat, g, w, h, dict(radius=4, gamma=1.0))
    ref = temporal.rectify_reference(image2, se2, feat, g, w, h, dict(radius=4, gamma=1.0))
    _close(mixed[0], ref[0], np.ones((h, w), dtype=bool), 32.0, "non-finite taps in the window", rho=True)
