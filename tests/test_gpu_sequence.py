"""Camera sequences end to end on the GPU (ptmi/temporal.py render_sequence, pt --frames): the
accumulated last frame of an orbit is closer to the converged frame than the plain last frame is, with
and without the spatial filter, and the CLI writes the frames render_sequence computes.

Reference scene, 64 x 48, 8 frames x 8 spp, 1.5 degrees per frame, seed streams 300 + k; the converged
frame is 1024 spp at the last camera; RMSE over the hit pixels.  Measured on an MI355X
(profiles/temporal/SUMMARY.md): RMSE accumulated / plain = 0.259 (0.08680 against 0.33542), accumulated +
filtered / filtered alone = 0.626 (0.06574 against 0.10499), mean history length 7.933 of 8.  Asserted: each
ratio below the midpoint between the measured value and 1 (0.63 and 0.813), so a regression to "no
history used" (ratio 1) fails, and a mean history length above 4."""
import os
import subprocess

import numpy as np
import pytest

from ptmi import api, denoise, temporal
from tests.scene_inputs import scene_inputs
from tests.test_host import _clamp, _read_png

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")
W, H, FRAMES, SPP, STEP, SEED, CONVERGED = 64, 48, 8, 8, 1.5, 300, 1024
MEASURED_TEMPORAL, MEASURED_DENOISED, MEASURED_HISTORY = 0.259, 0.626, 7.933


def _rmse(a, b, hit):
    a, b = (x.reshape(-1, 4)[hit][:, :3] for x in (a, b))
    return float(np.sqrt(((a - b) ** 2).mean()))


def test_accumulated_frame_is_closer_to_the_converged_one():
    import torch
    objs, tris, grps, cam = scene_inputs("reference", W, H)
    cams = [temporal.orbit_camera(cam, k * STEP) for k in range(FRAMES)]
    sc = api.Scene(0, objs, tris, grps, cam)
    last = None
    for last in temporal.render_sequence(sc, cams, SPP, SEED, temporal=True, denoise=True):
        pass
    torch.cuda.synchronize()
    spatial, _, _ = denoise.denoise_frame(sc, last["image"], last["se"])  # the same last frame, no history
    kw = dict(dtype=torch.float64, device="cuda")
    seeds, sums, ref = torch.empty(W * H, **kw), torch.empty(W * H * 4, **kw), torch.empty(W * H * 4, **kw)
    api.fill_seeds(seeds.data_ptr(), W * H, SEED + 1000)
    sc.render(CONVERGED, 0, CONVERGED, seeds.data_ptr(), sums.data_ptr())  # the scene stands at the last camera
    sc.finalize(sums.data_ptr(), ref.data_ptr(), CONVERGED)
    torch.cuda.synchronize()
    sc.close()
    f = {k: v.cpu().numpy() for k, v in last.items()}
    ref, spatial = ref.cpu().numpy(), spatial.cpu().numpy()
    hit = f["feat"].reshape(-1, 12)[:, 7] >= 0
    n = f["hist"].reshape(-1, 8)[hit, 4]
    e_plain, e_acc = _rmse(f["image"], ref, hit), _rmse(f["accumulated"], ref, hit)
    e_spatial, e_both = _rmse(spatial, ref, hit), _rmse(f["out"], ref, hit)
    print("RMSE against %d spp over %d hit pixels: plain %d spp %.5f, accumulated %.5f (ratio %.3f); "
          "filtered alone %.5f, accumulated + filtered %.5f (ratio %.3f); mean history length %.3f (max %.3f); "
          "rms se plain %.5f accumulated %.5f" %
          (CONVERGED, int(hit.sum()), SPP, e_plain, e_acc, e_acc / e_plain, e_spatial, e_both, e_both / e_spatial,
           n.mean(), n.max(), np.sqrt((f["se"][hit] ** 2).mean()), np.sqrt((f["accumulated_se"][hit] ** 2).mean())))
    assert e_acc < e_plain and e_both < e_spatial
    assert e_acc / e_plain < 0.5 * (MEASURED_TEMPORAL + 1.0)
    assert e_both / e_spatial < 0.5 * (MEASURED_DENOISED + 1.0)
    assert n.mean() > 4.0


def test_cli_sequence_writes_the_frames_render_sequence_computes(tmp_path):
    import torch
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    frames, spp, step, seed = 3, 4, 2.0, 77
    png = tmp_path / "turn.png"
    cmd = [PT, "--scene", "reference", "--width", str(W), "--height", str(H), "--samples", str(spp), "--frames",
           str(frames), "--orbit-step", str(step), "--temporal", "--seed", str(seed), "--out", str(png)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    names = [tmp_path / ("turn.%04d.png" % k) for k in range(frames)]
    assert sorted(p.name for p in tmp_path.iterdir()) == [p.name for p in names]
    got = [_read_png(str(p)) for p in names]
    assert all(g.shape[:2] == (H, W) for g in got)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    objs, tris, grps, cam = scene_inputs("reference", W, H)
    sc = api.Scene(0, objs, tris, grps, cam)
    cams = [temporal.orbit_camera(cam, k * step) for k in range(frames)]
    for k, f in enumerate(temporal.render_sequence(sc, cams, spp, seed, temporal=True)):
        torch.cuda.synchronize()
        want = _clamp(f["out"].cpu().numpy().reshape(H, W, 4)[..., :3])
        assert np.array_equal(got[k][..., :3], want), "frame %d" % k
    sc.close()


def test_cli_temporal_needs_a_sequence():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--scene", "reference", "--samples", "4", "--temporal"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--frames" in r.stderr
