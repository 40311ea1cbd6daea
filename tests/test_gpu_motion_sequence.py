"""A moving object through render_sequence(objects=...) and the CLI: the reference scene at 64 x 48, 8 frames
of 8 spp with different seed streams, the larger ball (object 7) translated by 0.05 in x per frame (about
2.3 pixels; from x = 0 to 0.35, inside the box), the camera fixed.

Compared over the ball's pixels in the last frame, as orderings against the existing function on the same
frames -- not fixed numbers:
  * the mean history length with ptmi_reproject_motion exceeds that of ptmi_reproject chained over the
    same frames (the parent's behaviour: it looks each point up where it is now, so the pixels the ball
    newly covers reset, and the others pass the tests only where the wrong surface point is close);
  * against a 1024-spp frame of the last state, the RMSE of the motion-accumulated frame is below the
    plain last frame's and below the static-reprojection result's.
Measured on an MI355X (profiles/motion/SUMMARY.md): 183 ball pixels; mean history length 8.000 with the motion,
2.098 with ptmi_reproject; RMSE 0.0689 with the motion, 0.2223 the plain last frame, 0.1795 the static reprojection.

One CLI run of --move-object at 16 x 12 checks the frames written and the usage errors."""
import os
import subprocess

import numpy as np
import pytest

from ptmi import api, geom, temporal
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")
W, H, FRAMES, SPP, BALL, STEP, SEED = 64, 48, 8, 8, 7, 0.05, 4100


def test_moving_ball_accumulates_with_its_motion():
    import torch
    objs, tris, grps, cam = scene_inputs("reference", W, H)
    frames = [temporal.move_object(objs, BALL, geom.translate(k * STEP, 0.0, 0.0)) for k in range(FRAMES)]
    cams = [cam] * FRAMES
    sc = api.Scene(0, objs, tris, grps, cam)
    n = W * H
    kw = dict(dtype=torch.float64, device="cuda")
    # with the motion: the sequence as the library runs it
    last = None
    for f in temporal.render_sequence(sc, cams, SPP, SEED, temporal=True, objects=frames):
        last = f
    torch.cuda.synchronize()
    moved_hist = last["hist"].cpu().numpy().reshape(-1, 8)
    moved = last["accumulated"].cpu().numpy().reshape(-1, 4)[:, :3]
    plain = last["image"].cpu().numpy().reshape(-1, 4)[:, :3]
    feat = last["feat"].cpu().numpy().reshape(-1, 12)
    # the parent's behaviour on the same frames (same objects, seeds and renders): ptmi_reproject chained
    hist = [torch.empty(n * api.HISTORY_DOUBLES, **kw) for _ in range(2)]
    acc = torch.empty(n * 4, **kw)
    prev_feat = torch.empty(n * api.FEATURE_DOUBLES, **kw)
    for k, f in enumerate(temporal.render_sequence(sc, cams, SPP, SEED, temporal=False, objects=frames)):
        api.reproject(f["image"].data_ptr(), f["se"].data_ptr(), f["feat"].data_ptr(), hist[(k - 1) & 1].data_ptr() if k else 0,
                      prev_feat.data_ptr() if k else 0, cam if k else None, W, H, hist[k & 1].data_ptr(),
                      out_rgba_ptr=acc.data_ptr())
        torch.cuda.synchronize()
        if k == FRAMES - 1:
            assert np.array_equal(f["image"].cpu().numpy().reshape(-1, 4)[:, :3], plain), "the two runs render alike"
        prev_feat.copy_(f["feat"])
    static_hist = hist[(FRAMES - 1) & 1].cpu().numpy().reshape(-1, 8)
    static = acc.cpu().numpy().reshape(-1, 4)[:, :3]
    # the converged frame of the last state
    sc.set_objects(frames[-1])
    seeds, sums, truth = torch.empty(n, **kw), torch.empty(n * 4, **kw), torch.empty(n * 4, **kw)
    api.fill_seeds(seeds.data_ptr(), n, SEED + 1000)
    sc.render(1024, 0, 1024, seeds.data_ptr(), sums.data_ptr())
    sc.finalize(sums.data_ptr(), truth.data_ptr(), 1024)
    torch.cuda.synchronize()
    truth = truth.cpu().numpy().reshape(-1, 4)[:, :3]
    sc.close()
    ball = feat[:, 7] == BALL
    assert ball.sum() >= 100, ball.sum()
    rmse = lambda a: float(np.sqrt(np.mean((a[ball] - truth[ball]) ** 2)))  # noqa: E731
    n_moved, n_static = float(moved_hist[ball, 4].mean()), float(static_hist[ball, 4].mean())
    e_moved, e_plain, e_static = rmse(moved), rmse(plain), rmse(static)
    print("ball pixels %d; mean history length: motion %.3f, static reprojection %.3f; RMSE against 1024 spp: motion %.5f, "
          "plain last frame %.5f, static reprojection %.5f" % (ball.sum(), n_moved, n_static, e_moved, e_plain, e_static))
    assert n_moved > n_static
    assert e_moved < e_plain and e_moved < e_static
    # Off the ball the two runs agree bit for bit: a tap is accepted only on equal ids, so the ball's history never
    # reaches another object's pixels, and what stands still takes ptmi_reproject's own path.
    assert np.array_equal(moved_hist[~ball], static_hist[~ball])


def test_cli_moves_an_object(tmp_path):
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    png = tmp_path / "move.png"
    base = [PT, "--scene", "reference", "--width", "16", "--height", "12", "--samples", "4", "--seed", "5", "--out", str(png)]
    r = subprocess.run(base + ["--frames", "3", "--move-object", str(BALL), "--move-step", "0.1,0,0", "--temporal"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = ["move.%04d.png" % k for k in range(3)]
    assert sorted(p.name for p in tmp_path.iterdir()) == names
    data = [(tmp_path / name).read_bytes() for name in names]
    assert all(len(d) > 100 for d in data) and data[0] != data[1] and data[1] != data[2]
    for extra in (["--move-object", "7", "--move-step", "0.1,0,0"], ["--frames", "1", "--move-object", "7", "--move-step", "0.1,0,0"],
                  ["--frames", "3", "--move-object", "7"], ["--frames", "3", "--move-step", "0.1,0,0"],
                  ["--frames", "3", "--move-object", "8", "--move-step", "0.1,0,0"],
                  ["--frames", "3", "--move-object", "-1", "--move-step", "0.1,0,0"],
                  ["--frames", "3", "--move-object", "7", "--move-step", "0.1,0"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage:" in r.stderr, extra
        assert "--move-" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == names  # the refused runs wrote nothing
