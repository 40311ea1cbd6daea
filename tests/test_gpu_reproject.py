"""The device temporal-accumulation kernel (ptmi_reproject) against its numpy statement (ptmi/temporal.py
reproject_reference) on real renders: 4 spp per frame, a different seed stream per frame, three frames
chained so that real history (N > 1, fractional N, non-trivial variances) is read.

Cases: reference 36 x 20 with orbit steps of 0, 3 and 40 degrees per frame, teapot 28 x 20 with 3 degrees.

Tolerance.  Every operation of the kernel is an IEEE FP64 add, multiply, divide, square root or floor in
the order the numpy statement gives, and the matrix T is computed on the host by the same cofactor
formulas; the compilers may still round u, v differently in the last bits (the host inverse), and the
outputs are continuous in them: bilinear weights go to 0 where the floor flips.  Asserted: |device -
numpy| <= 1e-9 x the frame's largest channel value for colour and variance, and 1e-9 x max_history for N
-- about 1000 x the rounding one derives (a few 1e-13 of the scale); a wrong tap, weight or test moves a
pixel by its noise level, ~1e-2.  Measured on an MI355X: the device's bits equal numpy's in every case, difference 0
(profiles/temporal/SUMMARY.md).

A pixel is left out only when a discontinuous decision of the numpy statement lies within 1e-9 relative
of its threshold (temporal.undecided); at most 1 % of a frame may be.  tests/test_temporal_reference.py
checks on the CPU that the statement alone stays within that cap on these views."""
import numpy as np
import pytest

from ptmi import api, temporal
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu
CASES = (("reference", 36, 20, 0.0), ("reference", 36, 20, 3.0), ("reference", 36, 20, 40.0), ("teapot", 28, 20, 3.0))
SPP, FRAMES, CANARY, PAD = 4, 3, -12345.0, 64
_cache = {}


def _frames(scene, w, h, step):
    """Per frame (camera, image, se, feat) as numpy arrays: rendered once per case."""
    import torch
    key = (scene, w, h, step)
    if key not in _cache:
        objs, tris, grps, cam = scene_inputs(scene, w, h)
        cams = [temporal.orbit_camera(cam, k * step) for k in range(FRAMES)]
        sc = api.Scene(0, objs, tris, grps, cam)
        out = []
        for c, f in zip(cams, temporal.render_sequence(sc, cams, SPP, 900, temporal=False, chunks=2 if tris.size else 0)):
            torch.cuda.synchronize()
            out.append((c, f["image"].cpu().numpy(), f["se"].cpu().numpy(), f["feat"].cpu().numpy()))
        sc.close()
        _cache[key] = out
    return _cache[key]


def _device(image, se, feat, prev, w, h, params=None, want_rgba=True, want_se=True):
    """One ptmi_reproject call: (hist, out_rgba or None, out_se or None) with a canary behind every output."""
    import torch
    kw = dict(dtype=torch.float64, device="cuda")
    up = lambda a: torch.tensor(np.ascontiguousarray(a).reshape(-1), **kw)  # noqa: E731
    d_img, d_se, d_feat = up(image), up(se), up(feat)
    prev_hist, prev_feat, prev_cam = (up(prev[0]), up(prev[1]), prev[2]) if prev else (None, None, None)
    n = w * h
    bufs = [torch.full((n * k + PAD,), CANARY, **kw) for k in (api.HISTORY_DOUBLES, 4, 1)]
    api.reproject(d_img.data_ptr(), d_se.data_ptr(), d_feat.data_ptr(), prev_hist.data_ptr() if prev else 0,
                  prev_feat.data_ptr() if prev else 0, prev_cam, w, h, bufs[0].data_ptr(),
                  out_rgba_ptr=bufs[1].data_ptr() if want_rgba else 0, out_se_ptr=bufs[2].data_ptr() if want_se else 0,
                  params=params)
    torch.cuda.synchronize()
    res = [b.cpu().numpy() for b in bufs]
    for b, k, used in zip(res, (api.HISTORY_DOUBLES, 4, 1), (True, want_rgba, want_se)):
        assert np.all(b[n * k:] == CANARY), "the canary behind an output was overwritten"
        if not used:
            assert np.all(b == CANARY), "an output that was not asked for was written"
    return res[0][:n * 8], (res[1][:n * 4] if want_rgba else None), (res[2][:n] if want_se else None)


def _compare(dev, ref, info, w, h, params, label):
    """Device against numpy for one frame; returns the largest relative differences."""
    p = temporal.params_dict(params)
    keep = ~temporal.undecided(info, w, h, params).reshape(-1)
    left_out = int((~keep).sum())
    hd, hr = dev[0].reshape(-1, 8), ref[0].reshape(-1, 8)
    fin = np.isfinite(hr[:, :4]).all(1)
    assert np.array_equal(hd[~fin], hr[~fin], equal_nan=True)  # pixels that are not finite: the input's bits
    m = keep & fin
    scale = np.abs(hr[fin, :3]).max()
    d_c = np.abs(hd[m, :3] - hr[m, :3]).max() / scale
    d_v = np.abs(hd[m, 3] - hr[m, 3]).max() / scale
    d_n = np.abs(hd[m, 4] - hr[m, 4]).max() / p["max_history"]
    print("%s: %d of %d pixels left out; max |device - numpy|: colour %.3e, variance %.3e of the largest channel, "
          "N %.3e of max_history; N in [%g, %g], %d pixels blended" %
          (label, left_out, w * h, d_c, d_v, d_n, hr[:, 4].min(), hr[:, 4].max(), int((hr[:, 4] > 1.0).sum())))
    assert left_out <= 0.01 * w * h
    assert d_c <= 1e-9 and d_v <= 1e-9 and d_n <= 1e-9
    assert np.all(hd[:, 5:] == 0.0)
    # the optional outputs are (c', 1) and sqrt(var') of the history, bit for bit
    assert np.array_equal(dev[1].reshape(-1, 4)[:, :3], hd[:, :3], equal_nan=True) and np.all(dev[1][3::4] == 1.0)
    assert np.array_equal(dev[2], np.sqrt(hd[:, 3]), equal_nan=True)
    return d_c, d_v, d_n


@pytest.mark.parametrize("scene,w,h,step", CASES)
def test_chained_frames_match_numpy(scene, w, h, step):
    frames = _frames(scene, w, h, step)
    prev, blended = None, 0
    for k, (cam, image, se, feat) in enumerate(frames):
        dev = _device(image, se, feat, prev, w, h)
        again = _device(image, se, feat, prev, w, h)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(dev, again)), "two identical calls differ"
        ref = temporal.reproject_reference(image, se, feat, prev[0] if prev else None, prev[1] if prev else None,
                                           prev[2] if prev else None, w, h, details=True)
        _compare(dev, ref[:3], ref[3], w, h, None, "%s %dx%d step %g frame %d" % (scene, w, h, step, k))
        n = dev[0].reshape(-1, 8)[:, 4]
        if k == 0:
            fin = np.isfinite(image.reshape(-1, 4)[:, :3]).all(1) & np.isfinite(se)
            assert np.all(n[fin] == 1.0) and np.all(n[~fin] == 0.0)  # prev_hist_dev == NULL
        blended = int((n > 1.0).sum())
        prev = (dev[0], feat, cam)  # the device's own history feeds the next frame on both sides
    if step < 10.0:
        assert blended > 0.5 * w * h, "a small step keeps most pixels' history"
        assert (n > 2.0).any(), "the third frame read history with N > 1"


def test_parameters_reach_the_kernel():
    scene, w, h, step = CASES[1]
    frames = _frames(scene, w, h, step)
    hist0 = _device(*frames[0][1:], None, w, h)[0]
    prev = (hist0, frames[0][3], frames[0][0])
    cam, image, se, feat = frames[1]
    for params in (dict(max_history=1), dict(normal_cos=0.9999, plane_dist=1e-4), dict(min_weight=0.9)):
        dev = _device(image, se, feat, prev, w, h, params)
        ref = temporal.reproject_reference(image, se, feat, prev[0], prev[1], prev[2], w, h, params, details=True)
        _compare(dev, ref[:3], ref[3], w, h, params, "reference %r" % (params,))
    one = _device(image, se, feat, prev, w, h, dict(max_history=1))[0].reshape(-1, 8)
    assert np.all(one[np.isfinite(one[:, :4]).all(1), 4] == 1.0)


def test_optional_outputs_and_defaults():
    scene, w, h, step = CASES[1]
    frames = _frames(scene, w, h, step)
    hist0 = _device(*frames[0][1:], None, w, h)[0]
    prev = (hist0, frames[0][3], frames[0][0])
    cam, image, se, feat = frames[1]
    full = _device(image, se, feat, prev, w, h)
    for want_rgba, want_se in ((False, False), (True, False), (False, True)):
        part = _device(image, se, feat, prev, w, h, want_rgba=want_rgba, want_se=want_se)
        assert np.array_equal(part[0], full[0], equal_nan=True)
        assert part[1] is None or np.array_equal(part[1], full[1], equal_nan=True)
        assert part[2] is None or np.array_equal(part[2], full[2], equal_nan=True)
    explicit = _device(image, se, feat, prev, w, h, api.ReprojectParams(32, 0, 0.9, 0.02, 0.05))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(explicit, full))
    # a first frame needs no previous records or camera; non-finite pixels get N = 0 and are no history
    image2, se2 = image.copy(), se.copy()
    image2[4 * 7 + 1], se2[11] = np.nan, np.inf
    first = _device(image2, se2, feat, None, w, h)[0].reshape(-1, 8)
    assert first[7, 4] == 0.0 and first[11, 4] == 0.0 and np.isnan(first[7, 1]) and first[11, 3] == np.inf
    nxt = _device(image, se, feat, (first.reshape(-1), feat, cam), w, h)
    ref = temporal.reproject_reference(image, se, feat, first.reshape(-1), feat, cam, w, h, details=True)
    _compare(nxt, ref[:3], ref[3], w, h, None, "after a frame with non-finite pixels")
    assert np.isfinite(nxt[0]).all()
