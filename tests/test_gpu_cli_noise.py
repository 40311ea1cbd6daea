"""End to end on the GPU: the CLI's noise target (pt --noise-target / --batch / --error-map) runs the
loop of ptmi/error.py render_to_noise through the C ABI.  A frame stopped early is not the frame of
`--samples <samples_done>` (fgi2 = seed / samples depends on the total), so the comparator is the
Python loop with the same seed stream, through the PNG clamp."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from ptmi import api, error
from tests.scene_inputs import scene_inputs
from tests.test_host import _clamp, _read_png

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")


def test_cli_noise_target_matches_python_loop(tmp_path):
    import torch
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    w, h, S, B, seed = 40, 24, 256, 32, 4242
    sc = api.Scene(0, *scene_inputs("reference", w, h))
    seeds = torch.empty(w * h, dtype=torch.float64, device="cuda")
    api.fill_seeds(seeds.data_ptr(), w * h, seed)
    _, _, _, hist = error.render_to_noise(sc, S, B, 0.0, seeds.data_ptr())
    target = 0.5 * (hist[2] + hist[3])  # between two batches of this frame's own history
    img, se, done, hist2 = error.render_to_noise(sc, S, B, target, seeds.data_ptr())
    sc.close()
    png, emap = tmp_path / "o.png", tmp_path / "se.raw"
    cmd = [PT, "--scene", "reference", "--width", str(w), "--height", str(h), "--samples", str(S), "--batch", str(B),
           "--noise-target", repr(target), "--error-map", str(emap), "--seed", str(seed), "--out", str(png)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"samples_done (\d+) relative_error (\S+)", r.stdout)
    assert m, r.stdout
    samples_done = int(m.group(1))
    assert samples_done % B == 0 and samples_done == done and samples_done < S
    assert abs(float(m.group(2)) - hist2[-1]) <= 1e-5 * hist2[-1] and float(m.group(2)) <= target
    img = img.cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(_read_png(str(png))[..., :3], _clamp(img[..., :3]))
    body = open(emap, "rb").read()
    assert len(body) == 16 + w * h * 3 * 4
    assert struct.unpack(">iiii", body[:16]) == (1, 0, w, h)
    px = np.frombuffer(body[16:], ">f4").reshape(h, w, 3)
    se32 = se.cpu().numpy().reshape(h, w).astype(np.float32)
    for c in range(3):
        assert np.array_equal(px[..., c], se32)
