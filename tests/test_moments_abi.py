"""The moment / error-map boundary on CPU (no GPU calls): include/ptmi.h declares
ptmi_scene_render_moments, ptmi_error_map and ptmi_accumulate, libptmi.so exports them, the
numpy statement of the error map (ptmi/error.py) gives hand-computed values, and the CLI's
usage text names its noise flags."""
import os
import re
import subprocess

import numpy as np
import pytest

from ptmi import api, error

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ptmi_scene_render_moments", "ptmi_error_map", "ptmi_accumulate")
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")


def test_header_declares_moment_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert set(NEW) <= set(api.EXPORTS)


def test_library_exports_moment_entry_points():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def test_error_map_reference_hand_values():
    """Three pixels in a row: not owned (n = 0), one sample (n = 1), and n = 4 with paths
    (1,0,0), (0,0,0), (1,0,0), (0,0,0): sums (2,0,0), sq 2, mean 0.5, d = 2/4 - 0.25 = 0.25,
    var = 0.25 * 4/3 = 1/3, se2 = 1/12."""
    sums = np.array([0, 0, 0, 0, 0.3, 0.2, 0.1, 1, 2, 0, 0, 4], dtype=np.float64)
    sq = np.array([0.0, 0.14, 2.0])
    se, tile_err, stats = error.error_map_reference(sums, sq, 3, 1)
    se2 = (0.25 * (4.0 / 3.0)) / 4.0
    assert se[0] == 0.0 and se[1] == np.inf and se[2] == np.sqrt(se2)
    assert tile_err.shape == (1,) and tile_err[0] == np.sqrt(se2 / 1.0)
    assert stats[0] == np.sqrt(se2) and stats[1] == np.sqrt(se2)
    assert stats[2] == ((0.5 + 0.0) + 0.0) / 3.0 and stats[3] == 1.0
    # cancellation: a constant pixel has d = 0 up to rounding, clamped at 0 from below
    v = 0.1
    sums = np.array([3 * v, 3 * v, 3 * v, 3], dtype=np.float64)
    sq = np.array([3 * ((v * v + v * v) + v * v) * (1 - 2.0 ** -50)])
    se, _, stats = error.error_map_reference(sums, sq, 1, 1)
    assert se[0] == 0.0 and stats[0] == 0.0 and stats[3] == 1.0


def test_error_map_reference_tiles_and_empty_frame():
    """9x9 pixels: four tiles in raster order, edge tiles with 8, 8 and 1 in-image pixels."""
    w = h = 9
    rng = np.random.RandomState(3)
    n = np.full(w * h, 5.0)
    rgb = rng.rand(w * h, 3) * 5
    sums = np.concatenate([rgb, n[:, None]], axis=1).reshape(-1)
    sq = (rgb ** 2).sum(axis=1) / 5 + rng.rand(w * h)
    se, tile_err, stats = error.error_map_reference(sums, sq, w, h)
    se2 = (se ** 2).reshape(h, w)
    for t, blk in enumerate((se2[:8, :8], se2[:8, 8:], se2[8:, :8], se2[8:, 8:])):
        assert np.isclose(tile_err[t], np.sqrt(blk.mean()), rtol=1e-13, atol=0)
    assert np.isclose(stats[0], np.sqrt(se2.mean()), rtol=1e-13, atol=0)
    assert stats[1] == se.max() and stats[3] == w * h
    se, tile_err, stats = error.error_map_reference(np.zeros(w * h * 4), np.zeros(w * h), w, h)
    assert not se.any() and not tile_err.any() and not stats.any()


def test_cli_usage_names_noise_flags():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("--noise-target", "--batch", "--error-map"):
        assert flag in text, text
    r = subprocess.run([PT, "--gpus", "2", "--noise-target", "0.1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--gpus 1" in r.stderr
