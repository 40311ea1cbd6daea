"""The feature-pass / denoiser boundary on CPU (no GPU calls): include/ptmi.h declares
ptmi_scene_features, ptmi_denoise and ptmi_denoise_work_bytes, libptmi.so exports them, the Python
binding's parameter record has the header's layout, and the CLI's usage text names its flags."""
import ctypes
import os
import re
import subprocess

import pytest

from ptmi import api

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ptmi_scene_features", "ptmi_denoise", "ptmi_denoise_work_bytes")
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")


def test_header_declares_denoise_entry_points():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert set(NEW) <= set(api.EXPORTS)
    assert re.search(r"#define\s+PTMI_FEATURE_DOUBLES\s+12\b", src) and api.FEATURE_DOUBLES == 12
    assert re.search(r"#define\s+PTMI_DENOISE_DEMODULATE\s+1u?\b", src) and api.DENOISE_DEMODULATE == 1


def test_library_exports_denoise_entry_points():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def test_work_bytes_and_params_layout():
    """ptmi_denoise_work_bytes touches no device: two (r, g, b, var) states of doubles.  The ctypes record
    is the header's struct: 4 + 4 + 8 + 8 + 4 + 4 bytes, and its defaults are the documented ones."""
    lib = api.load_library()
    assert lib.ptmi_denoise_work_bytes(1280, 960) == 1280 * 960 * 64
    assert lib.ptmi_denoise_work_bytes(19, 11) == 19 * 11 * 64
    assert lib.ptmi_denoise_work_bytes(65536, 65536) == 65536 * 65536 * 64  # (size_t, no 32-bit wrap)
    assert ctypes.sizeof(api.DenoiseParams) == 32
    assert [(n, getattr(api.DenoiseParams, n).offset) for n, _ in api.DenoiseParams._fields_] == \
        [("iterations", 0), ("flags", 4), ("sigma_l", 8), ("sigma_d", 16), ("normal_power", 24), ("reserved", 28)]
    p = api.DenoiseParams()
    assert (p.iterations, p.flags, p.sigma_l, p.sigma_d, p.normal_power, p.reserved) == (5, 1, 4.0, 0.01, 7, 0)
    assert api.denoise_params({"iterations": 3}).iterations == 3 and api.denoise_params(None) is None


def test_cli_usage_names_denoise_flags():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("--denoise", "--denoise-iters", "--features"):
        assert flag in text, text
    # flag misuse ends in the usage error before any device is touched
    for extra in (["--denoise"], ["--features", "x.raw"], ["--denoise", "--noise-target", "0.1"]):
        r = subprocess.run([PT, "--gpus", "2"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--gpus 1" in r.stderr and "usage:" in r.stderr
    for bad in ("0", "9", "-1"):
        r = subprocess.run([PT, "--denoise", "--denoise-iters", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--denoise-iters" in r.stderr
    r = subprocess.run([PT, "--denoise-iters", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--denoise" in r.stderr
