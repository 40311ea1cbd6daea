"""End to end on the GPU: pt --noise-target X --adaptive [--sample-map] runs the loop of
ptmi/error.py render_adaptive through the C ABI.  The comparator is the Python loop with the same
seed stream: the PNG through the clamp, the sample map as float32, and the two stdout lines."""
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


def test_cli_adaptive_matches_python_loop(tmp_path):
    import torch
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    w, h, S, B, seed = 44, 27, 128, 16, 4243
    sc = api.Scene(0, *scene_inputs("reference", w, h))
    seeds = torch.empty(w * h, dtype=torch.float64, device="cuda")
    api.fill_seeds(seeds.data_ptr(), w * h, seed)
    # a target some tiles meet after one batch and others never: between the frame's own extremes
    _, _, _, hist = error.render_adaptive(sc, S, B, 0.0, seeds.data_ptr())
    assert len(hist) == S // B
    target = hist[S // B // 2][2]
    img, se, counts, hist = error.render_adaptive(sc, S, B, target, seeds.data_ptr())
    sc.close()
    counts = counts.cpu().numpy()
    assert counts.min() < counts.max()
    png, smap = tmp_path / "o.png", tmp_path / "n.raw"
    cmd = [PT, "--scene", "reference", "--width", str(w), "--height", str(h), "--samples", str(S), "--batch", str(B),
           "--noise-target", repr(target), "--adaptive", "--sample-map", str(smap), "--seed", str(seed),
           "--out", str(png)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^samples_done (\d+) relative_error (\S+)$", r.stdout, re.M)
    assert m, r.stdout
    assert int(m.group(1)) == counts.max()
    assert abs(float(m.group(2)) - hist[-1][2]) <= 1e-5 * hist[-1][2]
    m = re.search(r"^adaptive mean_spp (\S+) tiles_at_max (\d+)$", r.stdout, re.M)
    assert m, r.stdout
    assert abs(float(m.group(1)) - counts.mean()) <= 1e-5 * counts.mean()
    tile_n = counts.reshape(h, w)[::8, ::8]  # one pixel per tile: a tile's pixels share their count
    assert int(m.group(2)) == int((tile_n == S).sum())
    img = img.cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(_read_png(str(png))[..., :3], _clamp(img[..., :3]))
    body = open(smap, "rb").read()
    assert len(body) == 16 + w * h * 3 * 4
    assert struct.unpack(">iiii", body[:16]) == (1, 0, w, h)
    px = np.frombuffer(body[16:], ">f4").reshape(h, w, 3)
    for c in range(3):
        assert np.array_equal(px[..., c], counts.reshape(h, w).astype(np.float32))
