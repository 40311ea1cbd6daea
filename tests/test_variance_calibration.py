"""The calibration of the variance estimate on the CPU alone, through the oracle and the numpy statement
(ptmi/temporal.py variance_reference): the check of the estimate that does not depend on the device kernel.

The sequence of tests/test_gpu_variance_sequence.py -- reference scene, 64 x 48, 16 frames x 1 spp on the
1.5-degree orbit, seed streams 7300 + k (``seeds`` restates ptmi_fill_seeds, so the oracle renders the device's
frames) -- with first-hit records from the brute-force comparator tests/features_ref.py and the moment history
chained through variance_reference.  The truth is the oracle's own: TRUTH = 64 samples of the last (and of the
first) camera rendered one by one, whose unbiased per-pixel sample variance, summed over the three channels, is
each pixel's one-sample variance.  Figure of merit, as on the device:
sqrt(mean(se_est^2) / mean(one-sample variance)) over the hit pixels.

Measured on the CPU (profiles/variance/SUMMARY.md): 1.012 on the last frame (90 % temporal estimates, mean moment
length 14.214) and 1.059 on frame 0 (99 % spatial), beside 1.011 and 1.063 on the MI355X against its 256-spp
truth.  Asserted: a band of a factor 2 around each measured value -- the estimate is pooled over ~3000 pixels, so
its own scatter is far below that; the band is there to catch a wrong formula, not to certify accuracy."""
import numpy as np

import pyoracle
from ptmi import layout, temporal
from tests.scene_inputs import scene_inputs
from tests.test_temporal_reference import records

W, H, FRAMES, STEP, SEED, TRUTH = 64, 48, 16, 1.5, 7300, 64
MEASURED_CPU, MEASURED_CPU_FIRST = 1.012, 1.059
_cache = {}


def seeds(n, stream):
    """ptmi_fill_seeds restated (csrc/ptmi_image_kernels.hip seeds_kernel): SplitMix64 of stream + golden * (i + 1),
    the top 53 bits as k / 2^53."""
    with np.errstate(over="ignore"):
        z = np.uint64(stream) + np.uint64(0x9E3779B97F4A7C15) * np.arange(1, n + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _one_sample_variance(objs, tris, grps, cam, stream):
    """Per pixel the unbiased sample variance, summed over r, g, b, of TRUTH samples rendered one by one."""
    sd = seeds(W * H, stream)
    c = np.stack([pyoracle.cpu_trace(objs, tris, grps, cam, TRUTH, sd, sample_begin=j, sample_end=j + 1)
                  .reshape(-1, 4)[:, :3] for j in range(TRUTH)])
    return c.var(axis=0, ddof=1).sum(-1)


def measure():
    if "m" in _cache:
        return _cache["m"]
    objs, tris, grps, cam0 = scene_inputs("reference", W, H)
    tris, grps = layout.pad_empty(tris, grps)
    cams = [temporal.orbit_camera(cam0, k * STEP) for k in range(FRAMES)]
    mom = prev_feat = prev_cam = None
    first = None
    for k, cam in enumerate(cams):
        feat = records(cam, "reference", W, H)
        rgba = pyoracle.cpu_trace(objs, tris, grps, cam, 1, seeds(W * H, SEED + k))
        mom, se_est = temporal.variance_reference(rgba, None, feat, mom, prev_feat, prev_cam, W, H)
        if k == 0:
            first = (feat, se_est, mom)
        prev_feat, prev_cam = feat, cam
    m = {}
    for name, (f, se_est, mm), cam, stream in (("last", (feat, se_est, mom), cams[-1], SEED + 1001),
                                               ("first", first, cams[0], SEED + 2001)):
        hit = f[:, 7] >= 0
        truth = _one_sample_variance(objs, tris, grps, cam, stream)
        src = mm.reshape(-1, 8)[hit, 5]
        m[name] = float(np.sqrt((se_est[hit] ** 2).mean() / truth[hit].mean()))
        m[name + "_temporal"], m[name + "_spatial"] = float((src == 1.0).mean()), float((src == 2.0).mean())
        m[name + "_N"] = float(mm.reshape(-1, 8)[hit, 4].mean())
    print("CPU calibration sqrt(mean se_est^2 / mean one-sample variance), %d-sample truth: last frame %.4f (temporal "
          "on %.3f of the hit pixels, mean moment length %.3f), frame 0 %.4f (spatial on %.3f)" %
          (TRUTH, m["last"], m["last_temporal"], m["last_N"], m["first"], m["first_spatial"]))
    _cache["m"] = m
    return m


def test_fill_seeds_restatement_is_in_range():
    s = seeds(1000, SEED)
    assert s.min() >= 0.0 and s.max() < 1.0 and len(np.unique(s)) == 1000
    assert np.array_equal(s * 2.0 ** 53, np.floor(s * 2.0 ** 53))


def test_cpu_calibration_of_the_estimate():
    m = measure()
    assert m["last_temporal"] > 0.8 and m["first_spatial"] > 0.8 and m["last_N"] > 8.0
    assert 0.5 * MEASURED_CPU < m["last"] < 2.0 * MEASURED_CPU
    assert 0.5 * MEASURED_CPU_FIRST < m["first"] < 2.0 * MEASURED_CPU_FIRST
