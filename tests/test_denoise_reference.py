"""Properties of the numpy statement of the a-trous filter (ptmi/denoise.py atrous_reference), on
synthetic 19 x 11 and 67 x 66 buffers (tests/denoise_synth.py): what the filter must keep exactly,
what it must never mix, and that with every guide weight at 1 one pass is the plain B3-spline blur."""
import numpy as np
import pytest

from ptmi import denoise
from tests import denoise_synth as synth

SIZES = synth.SIZES


def _run(rgba, se, feat, w, h, **params):
    out, out_se = denoise.atrous_reference(rgba.reshape(-1), se.reshape(-1), feat.reshape(-1), w, h, params or None)
    return out.reshape(h, w, 4), out_se.reshape(h, w)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("flags", (0, 1))
def test_constant_image_is_kept_bit_for_bit(w, h, flags):
    """Any variance, any guide weights: equal colours stay equal.  (Albedo 0.5: the division and the
    multiplication of the demodulation are exact.)"""
    rng = np.random.RandomState(3)
    rgba = synth.frame((0.3, 0.7, 0.123456789), w, h)
    se = rng.rand(h, w) * 2.0
    feat = synth.plane_features(w, h, albedo=(0.5, 0.5, 0.5))
    feat[..., 4:7] = rng.randn(h, w, 3)  # arbitrary normals and depths: the weights vary, the colour cannot
    feat[..., 3] = 1.0 + rng.rand(h, w)
    out, out_se = _run(rgba, se, feat, w, h, flags=flags)
    assert np.array_equal(out, rgba)
    assert np.isfinite(out_se).all()


@pytest.mark.parametrize("w,h", SIZES)
def test_two_planes_keep_their_colours(w, h):
    """Normals 90 degrees apart: w_n is 0 across the seam, so neither constant colour moves."""
    x0 = w // 2
    feat = synth.plane_features(w, h)
    feat[:, x0:] = synth.plane_features(w, h, normal=(1.0, 0.0, 0.0), oid=1.0)[:, x0:]
    rgb = np.where((np.arange(w) >= x0)[None, :, None], (0.9, 0.1, 0.4), (0.2, 0.6, 0.05)) * np.ones((h, w, 3))
    rgba = synth.frame(rgb, w, h)
    se = np.full((h, w), 0.25)
    for flags in (0, 1):
        out, _ = _run(rgba, se, feat, w, h, flags=flags)
        assert np.array_equal(out, rgba)


@pytest.mark.parametrize("w,h", SIZES)
def test_variance_never_grows_on_a_flat_region(w, h):
    """A flat region with one variance everywhere: var' = var * sum(w^2) / sum(w)^2 <= var at every pixel,
    the corners included, pass after pass.  With a variance that differs from pixel to pixel a quiet
    pixel may take some from its neighbours, but none can exceed the largest one going in."""
    rng = np.random.RandomState(5)
    feat = synth.plane_features(w, h)
    rgba = synth.frame(0.5 + 0.05 * rng.randn(h, w, 3), w, h)
    for iters in (1, 2, 5):
        _, out_se = _run(rgba, np.full((h, w), 0.5), feat, w, h, iterations=iters, flags=0)
        assert np.all(out_se <= 0.5) and out_se.max() < 0.5
    se = 0.1 + rng.rand(h, w)
    prev = se.max()
    for iters in (1, 5):
        _, out_se = _run(rgba, se, feat, w, h, iterations=iters, flags=0)
        assert out_se.max() < prev
        prev = out_se.max()


@pytest.mark.parametrize("w,h", SIZES)
def test_nan_pixel_passes_through_and_poisons_nothing(w, h):
    rgba, se, feat, marks = synth.mixed_case(w, h)
    out, out_se = _run(rgba, se, feat, w, h)
    bad = np.zeros((h, w), dtype=bool)
    bad[marks["nan"]] = bad[marks["inf"]] = True
    # the two pixels come back as they went in, bit for bit (NaN included)
    assert np.array_equal(out[bad], rgba[bad], equal_nan=True)
    assert np.array_equal(out_se[bad], se[bad], equal_nan=True)
    assert np.isfinite(out[~bad]).all() and np.isfinite(out_se[~bad]).all()
    assert np.all(out[..., 3] == 1.0)
    # and nothing else saw them: the same frame with those two pixels repaired gives the same neighbours
    # only where no tap reaches them; within reach the results differ, so compare against a frame where
    # the bad pixels are finite but far outside any weight (a miss among hits)
    rgba2, se2, feat2 = rgba.copy(), se.copy(), feat.copy()
    for m in (marks["nan"], marks["inf"]):
        rgba2[m][:3] = 0.0
        se2[m] = 0.0
        feat2[m] = synth.miss_features(1, 1)[0, 0]
    out2, out_se2 = _run(rgba2, se2, feat2, w, h)
    assert np.array_equal(out[~bad], out2[~bad]) and np.array_equal(out_se[~bad], out_se2[~bad])


@pytest.mark.parametrize("w,h", SIZES)
def test_hits_and_misses_do_not_mix(w, h):
    """Hits red, misses blue, both noisy in their own channel only: after five passes no hit has any
    blue and no miss any red."""
    rng = np.random.RandomState(9)
    feat = synth.plane_features(w, h)
    miss = np.zeros((h, w), dtype=bool)
    miss[:, : w // 3] = True
    miss[h // 2:, w // 2:] = True
    feat[miss] = synth.miss_features(1, 1)[0, 0]
    rgb = np.zeros((h, w, 3))
    rgb[..., 0] = np.where(miss, 0.0, 0.5 + 0.3 * rng.rand(h, w))
    rgb[..., 2] = np.where(miss, 0.5 + 0.3 * rng.rand(h, w), 0.0)
    out, _ = _run(synth.frame(rgb, w, h), np.full((h, w), 0.2), feat, w, h)
    assert np.all(out[miss][:, 0] == 0.0) and np.all(out[~miss][:, 2] == 0.0)
    # both sides were filtered: their own channel's spread fell
    assert out[~miss][:, 0].std() < 0.5 * rgb[~miss][:, 0].std()
    assert out[miss][:, 2].std() < 0.5 * rgb[miss][:, 2].std()


@pytest.mark.parametrize("w,h", SIZES)
def test_one_pass_without_guides_is_the_b_spline_blur(w, h):
    """One plane, huge sigmas: every weight is h[dx] h[dy] (exp(-x) with x < 1e-25 is 1.0), so one pass
    is the 5 x 5 B3-spline blur renormalised over the in-image taps, computed here independently (a
    dense loop over pixels and taps).  Tolerance 1e-14 relative to the largest value: two differently
    ordered sums of 25 terms of size <= 1."""
    rng = np.random.RandomState(13)
    feat = synth.plane_features(w, h)
    rgb = rng.rand(h, w, 3)
    se = 0.1 + rng.rand(h, w)
    out, out_se = _run(synth.frame(rgb, w, h), se, feat, w, h, iterations=1, flags=0, sigma_l=1e30, sigma_d=1e30)
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    blur, var = np.zeros((h, w, 3)), np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            sw = sc = sv = 0.0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        wt = k[dy + 2] * k[dx + 2]
                        sw += wt
                        sc = sc + wt * rgb[y + dy, x + dx]
                        sv += wt * wt * se[y + dy, x + dx] ** 2
            blur[y, x], var[y, x] = sc / sw, sv / (sw * sw)
    assert np.abs(out[..., :3] - blur).max() <= 1e-14
    assert np.abs(out_se - np.sqrt(var)).max() <= 1e-14 * se.max()


def test_parameters_are_checked():
    w, h = SIZES[0]
    rgba, se, feat, _ = synth.mixed_case(w, h)
    for bad in (dict(iterations=0), dict(iterations=9), dict(flags=2), dict(normal_power=17), dict(sigma_l=-1.0),
                dict(sigma_d=float("nan"))):
        with pytest.raises(ValueError):
            _run(rgba, se, feat, w, h, **bad)
    assert denoise.params_dict(None) == dict(iterations=5, flags=1, sigma_l=4.0, sigma_d=0.01, normal_power=7)
