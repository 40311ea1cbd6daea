"""A lighting change through render_sequence(rectify=...) and the CLI: the reference scene at 64 x 48, 12
frames of 8 spp with seed streams s + k, the camera fixed; from frame 8 on every emissive object's emission
is a third of what it was (Scene.set_objects -- geometry, and so every first-hit record, unchanged: the
plain accumulation finds a history for every pixel and trusts it).

Against a 1024-spp frame of the dimmed scene, over the pixels with a first hit, on frame 11:
  (a) the rectified accumulation, (b) the plain accumulation (rectify=None), (c) the 8-spp frame itself.
Asserted, as orderings on the same frames: RMSE (a) < (b) and (a) < (c); the mean history length of (a) is
below (b)'s; the mean rho of frame 8 is below frame 7's.

The static control runs the same 12 frames without the change against a 1024-spp frame of the unchanged
scene: there rectification can only lose (it forgets history that was right), and RMSE (a) may exceed (b) by
at most twice the excess measured when this test was written, and never by more than 10 %.

Measured on an MI355X (profiles/rectify/SUMMARY.md), frame 11 over the 3072 hit pixels: RMSE (a) 0.0740,
(b) 0.1650, (c) 0.1162; mean N 7.45 against 12.00; mean rho 0.9989 on frame 7, 0.5502 on frame 8, 0.936-0.976
after it.  Static control: RMSE (a) / (b) per frame between 0.9999 and 1.0032 (frame 11: 0.10434 / 0.10401), mean
rho 0.997, mean N 11.90 against 12.00.  (a) < (c) held on that first measurement, so it is asserted.

One CLI run of --rectify with --emission-step at 16 x 12 checks the frames written and the usage errors."""
import os
import subprocess

import numpy as np
import pytest

from ptmi import api, temporal
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")
W, H, FRAMES, SPP, SEED, DIM_AT, DIM = 64, 48, 12, 8, 5200, 8, 1.0 / 3.0
STATIC_EXCESS = 0.0064  # RMSE (a) / RMSE (b) - 1 allowed in the static control: 2 x the 0.0032 measured (cap: 10 %)


def _dimmed(objs):
    out = np.ascontiguousarray(objs).copy()
    lit = (np.asarray(out["emission"])[:, :3] != 0.0).any(1)
    assert lit.any(), "the scene has a light"
    em = np.asarray(out["emission"]).copy()
    em[lit, :3] = em[lit, :3] * DIM
    out["emission"] = em
    return out


def _truth(sc, objs):
    import torch
    n = W * H
    kw = dict(dtype=torch.float64, device="cuda")
    sc.set_objects(objs)
    seeds, sums, truth = torch.empty(n, **kw), torch.empty(n * 4, **kw), torch.empty(n * 4, **kw)
    api.fill_seeds(seeds.data_ptr(), n, SEED + 1000)
    sc.render(1024, 0, 1024, seeds.data_ptr(), sums.data_ptr())
    sc.finalize(sums.data_ptr(), truth.data_ptr(), 1024)
    torch.cuda.synchronize()
    return truth.cpu().numpy().reshape(-1, 4)[:, :3]


def _run(sc, cam, objects, rectify):
    """Per frame: (accumulated rgb, plain rgb, N, rho or None, ids)."""
    import torch
    out = []
    for f in temporal.render_sequence(sc, [cam] * FRAMES, SPP, SEED, temporal=True, objects=objects, rectify=rectify):
        torch.cuda.synchronize()
        out.append((f["accumulated"].cpu().numpy().reshape(-1, 4)[:, :3], f["image"].cpu().numpy().reshape(-1, 4)[:, :3],
                    f["hist"].cpu().numpy().reshape(-1, 8)[:, 4], f["rho"].cpu().numpy() if "rho" in f else None,
                    f["feat"].cpu().numpy().reshape(-1, 12)[:, 7]))
    return out


def _rmse(a, truth, m):
    return float(np.sqrt(np.mean((a[m] - truth[m]) ** 2)))


def test_a_dimmed_light_is_noticed():
    objs, tris, grps, cam = scene_inputs("reference", W, H)
    dim = _dimmed(objs)
    seq = [objs] * DIM_AT + [dim] * (FRAMES - DIM_AT)
    sc = api.Scene(0, objs, tris, grps, cam)
    rect, plain = _run(sc, cam, seq, True), _run(sc, cam, seq, None)
    truth = _truth(sc, dim)
    still_r, still_p = _run(sc, cam, [objs] * FRAMES, True), _run(sc, cam, [objs] * FRAMES, None)
    truth0 = _truth(sc, objs)
    sc.close()
    hit = rect[-1][4] >= 0.0
    assert hit.sum() > 0.5 * W * H
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(rect, plain)), "the two runs render alike"
    assert all(r[3] is None for r in plain) and np.all(rect[0][3] == 1.0)
    e_a, e_b, e_c = _rmse(rect[-1][0], truth, hit), _rmse(plain[-1][0], truth, hit), _rmse(rect[-1][1], truth, hit)
    n_a, n_b = float(rect[-1][2][hit].mean()), float(plain[-1][2][hit].mean())
    rho = [float(r[3][hit].mean()) for r in rect]
    print("dimmed at frame %d, frame %d over %d hit pixels: RMSE against 1024 spp: rectified %.5f, plain accumulation %.5f, "
          "the %d-spp frame %.5f; mean N: rectified %.3f, plain %.3f" % (DIM_AT, FRAMES - 1, hit.sum(), e_a, e_b, SPP, e_c,
                                                                       n_a, n_b))
    print("mean rho per frame: " + " ".join("%.4f" % r for r in rho))
    print("RMSE per frame, rectified / plain: " + " ".join(
        "%.4f/%.4f" % (_rmse(a[0], truth if k >= DIM_AT else truth0, hit), _rmse(b[0], truth if k >= DIM_AT else truth0, hit))
        for k, (a, b) in enumerate(zip(rect, plain))))
    s_a, s_b = _rmse(still_r[-1][0], truth0, hit), _rmse(still_p[-1][0], truth0, hit)
    per_frame = [_rmse(a[0], truth0, hit) / _rmse(b[0], truth0, hit) for a, b in zip(still_r, still_p)]
    print("static control, frame %d: RMSE rectified %.5f, plain accumulation %.5f, ratio %.4f; mean N %.3f / %.3f; mean rho %.4f"
          % (FRAMES - 1, s_a, s_b, s_a / s_b, still_r[-1][2][hit].mean(), still_p[-1][2][hit].mean(),
             still_r[-1][3][hit].mean()))
    print("static control, ratio per frame: " + " ".join("%.4f" % r for r in per_frame))
    assert e_a < e_b and e_a < e_c
    assert n_a < n_b
    assert rho[DIM_AT] < rho[DIM_AT - 1]
    assert STATIC_EXCESS <= 0.10
    assert all(r <= 1.0 + STATIC_EXCESS for r in per_frame), per_frame


def test_cli_rectifies_a_sequence(tmp_path):
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    png = tmp_path / "dim.png"
    base = [PT, "--scene", "reference", "--width", "16", "--height", "12", "--samples", "4", "--seed", "5", "--out", str(png)]
    seq = ["--frames", "4", "--temporal"]
    r = subprocess.run(base + seq + ["--rectify", "--rectify-gamma", "2", "--rectify-radius", "2", "--emission-step", "0.25"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = ["dim.%04d.png" % k for k in range(4)]
    assert sorted(p.name for p in tmp_path.iterdir()) == names
    dimmed = [(tmp_path / name).read_bytes() for name in names]
    assert all(len(d) > 100 for d in dimmed)
    # the same sequence without the step: equal up to frame N / 2, different from it on
    r = subprocess.run(base + seq + ["--rectify", "--rectify-gamma", "2", "--rectify-radius", "2"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lit = [(tmp_path / name).read_bytes() for name in names]
    assert lit[:2] == dimmed[:2] and lit[2] != dimmed[2] and lit[3] != dimmed[3]
    for extra in (["--rectify"], ["--frames", "4", "--rectify"], seq + ["--rectify-gamma", "2"],
                  seq + ["--rectify", "--rectify-radius", "5"], seq + ["--rectify", "--rectify-gamma", "-1"],
                  ["--emission-step", "0.5"], seq + ["--emission-step", "-1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage:" in r.stderr, extra
    assert sorted(p.name for p in tmp_path.iterdir()) == names  # the refused runs wrote nothing
