"""The adaptive-sampling boundary on CPU (no GPU calls): include/ptmi.h declares
ptmi_scene_render_tiles, ptmi_select_tiles and ptmi_finalize_counts, libptmi.so exports them, the
numpy statements of the two small kernels (ptmi/error.py) give hand-computed values, and the CLI's
usage text names its adaptive flags."""
import os
import re
import subprocess

import numpy as np
import pytest

from ptmi import api, error

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ptmi_scene_render_tiles", "ptmi_select_tiles", "ptmi_finalize_counts")
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")


def test_header_declares_adaptive_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert set(NEW) <= set(api.EXPORTS)


def test_library_exports_adaptive_entry_points():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def test_select_tiles_reference_hand_values():
    """Errors of tiles 0..6: above, tie, NaN, +inf, below, above, -inf against threshold 1.0."""
    err = np.array([1.5, 1.0, np.nan, np.inf, 0.5, np.nextafter(1.0, 2.0), -np.inf])
    out, n = error.select_tiles_reference(err, None, 7, 1.0)
    assert out.dtype == np.uint32 and n == 3 and out.tolist() == [0, 3, 5]
    # the first four tiles only
    out, n = error.select_tiles_reference(err, None, 4, 1.0)
    assert n == 2 and out.tolist() == [0, 3]
    # an input list: candidate order is kept, not tile order; entries past n_in are not candidates
    out, n = error.select_tiles_reference(err, [5, 2, 1, 3, 4, 0, 6], 5, 1.0)
    assert n == 2 and out.tolist() == [5, 3]
    # a threshold of +inf keeps nothing (inf > inf is false), one of -inf everything but NaN and -inf
    assert error.select_tiles_reference(err, None, 7, np.inf)[1] == 0
    assert error.select_tiles_reference(err, None, 7, -np.inf)[0].tolist() == [0, 1, 3, 4, 5]
    # a NaN threshold keeps nothing
    assert error.select_tiles_reference(err, None, 7, np.nan)[1] == 0
    # empty input, with and without a list
    for lst in (None, [], [3, 0]):
        out, n = error.select_tiles_reference(err, lst, 0, 1.0)
        assert n == 0 and out.size == 0 and out.dtype == np.uint32


def test_finalize_counts_reference_hand_values():
    """Four pixels with counts 0 (sums 0), 0 (stray sums: still RGB 0), 4 and 3: the multiply by
    1.0 / n, not a division (2 * (1/3) and 2 / 3 differ in the last bit; 1 * (1/3) is 1/3)."""
    sums = np.array([0, 0, 0, 0, 7, 8, 9, 0, 2, 1, 0.5, 4, 2, 1, 5, 3], dtype=np.float64)
    out = error.finalize_counts_reference(sums)
    third = 1.0 / 3.0
    exp = [0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.25, 0.125, 1, 2 * third, third, 5 * third, 1]
    assert out.shape == (16,) and out.tolist() == exp
    assert 5 * third != 5.0 / 3.0  # (so the case tells the two apart)
    # a uniform count is ptmi_finalize's rule
    rng = np.random.RandomState(5)
    s = rng.rand(10, 4)
    s[:, 3] = 48
    out = error.finalize_counts_reference(s.reshape(-1)).reshape(10, 4)
    assert np.array_equal(out[:, :3], s[:, :3] * (1.0 / 48)) and np.all(out[:, 3] == 1.0)
    assert error.finalize_counts_reference(np.zeros(0)).size == 0


def test_cli_usage_names_adaptive_flags():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("--adaptive", "--sample-map"):
        assert flag in text, text
    r = subprocess.run([PT, "--adaptive"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--noise-target" in r.stderr
    for extra in (["--adaptive"], ["--adaptive", "--sample-map", "x.raw"]):
        r = subprocess.run([PT, "--gpus", "2", "--noise-target", "0.1"] + extra, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode != 0 and "--gpus 1" in r.stderr
    r = subprocess.run([PT, "--noise-target", "0.1", "--sample-map", "x.raw"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--adaptive" in r.stderr
