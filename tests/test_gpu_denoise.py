"""The device a-trous filter (ptmi_denoise) against its numpy statement (ptmi/denoise.py
atrous_reference), its argument checks, the end-to-end quality of render_denoised and the CLI.

Tolerance against numpy.  Every operation of the filter is an IEEE FP64 add, multiply, divide or
square root in a fixed order, identical on both sides, except exp: the device's and numpy's may
differ in the last bit.  So the constant image, pass-through pixels and alpha are compared for
equality, and everything else by the largest |device - numpy| relative to the frame's largest
channel value.  Measured on these inputs (MI355X): at most 3.276e-16 for the colour (teapot 28 x 20,
one pass, no demodulation) and 1.767e-16 for the standard error (synthetic 67 x 66) -- MEASURED_REL
below; the bound asserted is 100 x that, 3.3e-14, and never more than 1e-9: a wrong tap, weight or
order shows at 1e-3 or more.  End to end (test_denoised_frame_is_closer_to_the_converged_one): RMSE
ratio denoised / plain 0.396 on reference 64 x 48 (16 against 1024 spp), 0.481 on teapot 48 x 32 (16
against 512 spp); asserted only to be below 1."""
import os
import struct
import subprocess

import numpy as np
import pytest

from ptmi import api, denoise, layout
from tests import denoise_synth as synth
from tests.scene_inputs import scene_inputs
from tests.test_host import _clamp, _read_png

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")
MEASURED_REL = 3.3e-16  # largest |device - numpy| / max channel value over every case below (teapot, 1 pass: 3.276e-16)
BOUND = min(100 * MEASURED_REL, 1e-9)
_rendered_cache = {}


def _device(rgba, se, feat, w, h, params=None, variant=None):
    import torch
    kw = dict(dtype=torch.float64, device="cuda")
    d_rgba, d_se = torch.tensor(rgba.reshape(-1), **kw), torch.tensor(se.reshape(-1), **kw)
    d_feat = torch.tensor(feat.reshape(-1), **kw)
    lib = api.load_library()
    prev = lib.ptmi_diag_denoise_variant(variant) if variant is not None else None
    res = []
    try:
        for _ in range(2):
            out, out_se = torch.full((w * h * 4,), -3.0, **kw), torch.full((w * h,), -3.0, **kw)
            api.denoise(d_rgba.data_ptr(), d_se.data_ptr(), d_feat.data_ptr(), w, h, out.data_ptr(),
                        out_se_ptr=out_se.data_ptr(), params=params)
            torch.cuda.synchronize()
            res.append((out.cpu().numpy(), out_se.cpu().numpy()))
    finally:
        if prev is not None:
            lib.ptmi_diag_denoise_variant(prev)
    assert np.array_equal(res[0][0], res[1][0], equal_nan=True) and np.array_equal(res[0][1], res[1][1], equal_nan=True), \
        "two runs differ"
    return res[0]


def _compare(rgba, se, feat, w, h, params, label):
    out, out_se = _device(rgba, se, feat, w, h, params)
    ref, ref_se = denoise.atrous_reference(rgba, se, feat, w, h, params)
    assert np.all(out[3::4] == 1.0)
    special = ~np.isfinite(ref)
    assert np.array_equal(out[special], ref[special], equal_nan=True)
    sp_se = ~np.isfinite(ref_se)
    assert np.array_equal(out_se[sp_se], ref_se[sp_se], equal_nan=True)
    scale = np.abs(ref[~special]).max()
    rel = np.abs(out[~special] - ref[~special]).max() / scale
    rel_se = np.abs(out_se[~sp_se] - ref_se[~sp_se]).max() / max(np.abs(ref_se[~sp_se]).max(), 1e-300)
    print("%s %dx%d %r: max |device - numpy| / max value: colour %.3e, se %.3e" % (label, w, h, params, rel, rel_se))
    assert rel <= BOUND and rel_se <= BOUND
    return out, out_se


def _rendered(scene, w, h, S):
    import torch
    key = (scene, w, h, S)
    if key not in _rendered_cache:
        sc = api.Scene(0, *scene_inputs(scene, w, h))
        seeds = torch.tensor(layout.seeds_go_float64(w * h, 5), dtype=torch.float64, device="cuda")
        _, _, image, se, feat = denoise.render_denoised(sc, S, seeds.data_ptr())
        torch.cuda.synchronize()
        sc.close()
        _rendered_cache[key] = (image.cpu().numpy(), se.cpu().numpy(), feat.cpu().numpy())
    return _rendered_cache[key]


PARAMS = [dict(iterations=i, flags=f) for i in (1, 5) for f in (0, 1)]


@pytest.mark.parametrize("w,h", synth.SIZES)
@pytest.mark.parametrize("params", PARAMS)
def test_filter_matches_numpy_on_synthetic_buffers(w, h, params):
    rgba, se, feat, marks = synth.mixed_case(w, h)
    out, out_se = _compare(rgba, se, feat, w, h, params, "mixed")
    out, out_se = out.reshape(h, w, 4), out_se.reshape(h, w)
    for m in (marks["nan"], marks["inf"]):  # pass-through pixels: the input's bits
        assert np.array_equal(out[m][:3], rgba[m][:3], equal_nan=True) and out_se[m] == se[m]


@pytest.mark.parametrize("w,h", synth.SIZES)
def test_constant_image_is_exact(w, h):
    rng = np.random.RandomState(3)
    rgba = synth.frame((0.3, 0.7, 0.123456789), w, h)
    se = rng.rand(h, w) * 2.0
    feat = synth.plane_features(w, h, albedo=(0.5, 0.5, 0.5))
    feat[..., 4:7] = rng.randn(h, w, 3)
    feat[..., 3] = 1.0 + rng.rand(h, w)
    for flags in (0, 1):
        out, _ = _device(rgba, se, feat, w, h, dict(flags=flags))
        assert np.array_equal(out, rgba.reshape(-1))


@pytest.mark.parametrize("scene,w,h,S", (("reference", 36, 20, 13), ("teapot", 28, 20, 24)))
@pytest.mark.parametrize("params", PARAMS)
def test_filter_matches_numpy_on_rendered_frames(scene, w, h, S, params):
    image, se, feat = _rendered(scene, w, h, S)
    _compare(image, se, feat, w, h, params, scene)


def test_default_parameters_are_the_documented_ones():
    w, h = synth.SIZES[0]
    rgba, se, feat, _ = synth.mixed_case(w, h)
    a = _device(rgba, se, feat, w, h, None)
    b = _device(rgba, se, feat, w, h, api.DenoiseParams(5, 1, 4.0, 0.01, 7))
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("w,h", synth.SIZES)
def test_lds_and_gather_forms_give_the_same_bits(w, h):
    rgba, se, feat, _ = synth.mixed_case(w, h)
    a = _device(rgba, se, feat, w, h, None, variant=0)
    b = _device(rgba, se, feat, w, h, None, variant=1)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def test_argument_errors_launch_nothing():
    import torch
    w, h = 19, 11
    kw = dict(dtype=torch.float64, device="cuda")
    rgba, se, feat = torch.zeros(w * h * 4, **kw), torch.zeros(w * h, **kw), torch.zeros(w * h * 12, **kw)
    out, out_se = torch.full((w * h * 4,), -3.0, **kw), torch.full((w * h,), -3.0, **kw)
    work = torch.full((api.denoise_work_bytes(w, h) // 8,), -5.0, **kw)
    ok = dict(rgba_ptr=rgba.data_ptr(), se_ptr=se.data_ptr(), feat_ptr=feat.data_ptr(), w=w, h=h,
              out_ptr=out.data_ptr(), out_se_ptr=out_se.data_ptr(), work=work)
    bad = [dict(rgba_ptr=0), dict(se_ptr=0), dict(feat_ptr=0), dict(out_ptr=0), dict(params=dict(iterations=0)),
           dict(params=dict(iterations=9)), dict(work=work[:-1]), dict(out_ptr=rgba.data_ptr()), dict(w=0),
           dict(params=dict(flags=2)), dict(params=dict(sigma_l=float("nan")))]
    for change in bad:
        with pytest.raises(api.PtmiError) as e:
            api.denoise(**dict(ok, **change))
        assert e.value.code == api.PTMI_ERR_ARG, change
    lib = api.load_library()
    err = __import__("ctypes").create_string_buffer(256)
    rc = lib.ptmi_denoise(rgba.data_ptr(), se.data_ptr(), feat.data_ptr(), w, h, None, out.data_ptr(), None, None,
                          work.numel() * 8, None, err, len(err))
    assert rc == api.PTMI_ERR_ARG  # a NULL workspace
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((out_se == -3.0).all()) and bool((work == -5.0).all())
    assert bool((rgba == 0.0).all())
    sc = api.Scene(0, *scene_inputs("reference", w, h))
    with pytest.raises(api.PtmiError) as e:
        sc.features(0)
    assert e.value.code == api.PTMI_ERR_ARG
    sc.close()
    api.denoise(**ok)  # and the good call goes through
    torch.cuda.synchronize()
    assert bool((out[3::4] == 1.0).all())


@pytest.mark.parametrize("scene,w,h,lo,hi", (("reference", 64, 48, 16, 1024), ("teapot", 48, 32, 16, 512)))
def test_denoised_frame_is_closer_to_the_converged_one(scene, w, h, lo, hi):
    """The same seeds at `lo` and `hi` spp; over the hit pixels RMSE(denoised lo, hi) < RMSE(lo, hi)."""
    import torch
    sc = api.Scene(0, *scene_inputs(scene, w, h))
    seeds = torch.tensor(layout.seeds_go_float64(w * h, 77), dtype=torch.float64, device="cuda")
    den, den_se, noisy, se, feat = denoise.render_denoised(sc, lo, seeds.data_ptr())
    sums, ref = torch.empty(w * h * 4, dtype=torch.float64, device="cuda"), torch.empty(w * h * 4, dtype=torch.float64,
                                                                                        device="cuda")
    sc.render(hi, 0, hi, seeds.data_ptr(), sums.data_ptr())
    sc.finalize(sums.data_ptr(), ref.data_ptr(), hi)
    torch.cuda.synchronize()
    sc.close()
    hit = feat.cpu().numpy().reshape(w * h, 12)[:, 7] >= 0
    den, noisy, ref = (a.cpu().numpy().reshape(w * h, 4)[hit][:, :3] for a in (den, noisy, ref))
    e_den, e_noisy = np.sqrt(((den - ref) ** 2).mean()), np.sqrt(((noisy - ref) ** 2).mean())
    print("%s %dx%d: RMSE %d spp %.5f, denoised %.5f, ratio %.3f; rms se in %.5f out %.5f" %
          (scene, w, h, lo, e_noisy, e_den, e_den / e_noisy, float(se.square().mean().sqrt()),
           float(den_se.square().mean().sqrt())))
    assert e_den < e_noisy


def test_cli_denoise_matches_render_denoised(tmp_path):
    import torch
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    w, h, S, seed = 64, 48, 16, 4243
    sc = api.Scene(0, *scene_inputs("reference", w, h))
    seeds = torch.empty(w * h, dtype=torch.float64, device="cuda")
    api.fill_seeds(seeds.data_ptr(), w * h, seed)
    den, _, noisy, _, feat = denoise.render_denoised(sc, S, seeds.data_ptr())
    torch.cuda.synchronize()
    sc.close()
    png, fraw = tmp_path / "o.png", tmp_path / "f.raw"
    cmd = [PT, "--scene", "reference", "--width", str(w), "--height", str(h), "--samples", str(S), "--denoise",
           "--features", str(fraw), "--seed", str(seed), "--out", str(png)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    den, noisy = den.cpu().numpy().reshape(h, w, 4), noisy.cpu().numpy().reshape(h, w, 4)
    got = _read_png(str(png))[..., :3]
    assert np.array_equal(got, _clamp(den[..., :3]))
    assert not np.array_equal(got, _clamp(noisy[..., :3]))  # (the filter ran)
    body = open(fraw, "rb").read()
    assert len(body) == 16 + w * h * 3 * 4
    assert struct.unpack(">iiii", body[:16]) == (1, 0, w, h)
    px = np.frombuffer(body[16:], ">f4").reshape(h, w, 3)
    want = denoise.normal_image(feat.cpu().numpy(), w, h).reshape(h, w, 4)[..., :3]
    assert np.array_equal(px, want.astype(np.float32))
