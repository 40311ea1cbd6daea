"""The camera-update / temporal-accumulation boundary on CPU (no GPU calls): include/ptmi.h declares
ptmi_scene_set_camera and ptmi_reproject, libptmi.so exports them, the Python binding's parameter record
has the header's layout, every PTMI_ERR_ARG case of ptmi_reproject is refused before any device call
(the pointers below are never dereferenced), and the CLI refuses --temporal without a sequence."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ptmi import api, layout, temporal
from tests.scene_inputs import scene_inputs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ptmi_scene_set_camera", "ptmi_reproject")
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")
W, H = 36, 20


def test_header_declares_temporal_entry_points():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert set(NEW) <= set(api.EXPORTS)
    assert re.search(r"#define\s+PTMI_HISTORY_DOUBLES\s+8\b", src)
    assert api.HISTORY_DOUBLES == 8 and temporal.HISTORY_DOUBLES == 8
    # the two points the header must state
    assert "HOST-BLOCKING" in text and "different seeds" in text


def test_library_exports_temporal_entry_points():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def test_params_layout_and_defaults():
    """The ctypes record is the header's struct: 4 + 4 + 8 + 8 + 8 bytes; its defaults are the documented ones."""
    assert ctypes.sizeof(api.ReprojectParams) == 32
    assert [(n, getattr(api.ReprojectParams, n).offset) for n, _ in api.ReprojectParams._fields_] == \
        [("max_history", 0), ("flags", 4), ("normal_cos", 8), ("plane_dist", 16), ("min_weight", 24)]
    p = api.ReprojectParams()
    assert (p.max_history, p.flags, p.normal_cos, p.plane_dist, p.min_weight) == (32, 0, 0.9, 0.02, 0.05)
    assert temporal.DEFAULTS == dict(max_history=32, flags=0, normal_cos=0.9, plane_dist=0.02, min_weight=0.05)
    assert api.reproject_params({"max_history": 3}).max_history == 3 and api.reproject_params(None) is None


def _camera(w=W, h=H):
    return scene_inputs("reference", w, h)[3]


def test_reproject_argument_errors_need_no_device():
    """Fake, 16-byte-aligned addresses: an accepted call would fault, a refused one never touches them."""
    a = 0x100000  # (further apart than the largest buffer, 36 x 20 x 96 bytes)
    ok = dict(rgba_ptr=a, se_ptr=2 * a, feat_ptr=3 * a, prev_hist_ptr=4 * a, prev_feat_ptr=5 * a, prev_camera=_camera(),
              w=W, h=H, out_hist_ptr=6 * a, out_rgba_ptr=7 * a, out_se_ptr=8 * a)
    singular = _camera().copy()
    singular["inverse"] = np.zeros(16)
    nan_cam = _camera().copy()
    nan_cam["inverse"][5] = np.nan
    bad = [dict(rgba_ptr=0), dict(se_ptr=0), dict(feat_ptr=0), dict(out_hist_ptr=0),
           dict(prev_feat_ptr=0), dict(prev_camera=None),             # required once there is a history
           dict(w=0), dict(h=0),
           dict(params=dict(max_history=0)), dict(params=dict(max_history=65537)), dict(params=dict(flags=1)),
           dict(params=dict(normal_cos=-0.1)), dict(params=dict(normal_cos=float("nan"))),
           dict(params=dict(plane_dist=-1.0)), dict(params=dict(plane_dist=float("inf"))),
           dict(params=dict(min_weight=-0.5)), dict(params=dict(min_weight=float("nan"))),
           dict(out_hist_ptr=4 * a),                                   # aliased history
           dict(out_hist_ptr=4 * a + 16), dict(out_hist_ptr=4 * a - 16),  # ... overlapping, not equal
           dict(out_hist_ptr=4 * a + W * H * 64 - 16),                 # ... by its last 16 bytes
           dict(out_rgba_ptr=a), dict(out_se_ptr=2 * a),               # no in-place outputs
           dict(out_rgba_ptr=6 * a + 32), dict(out_se_ptr=7 * a + 8),  # an output inside another output
           dict(out_hist_ptr=3 * a + 96), dict(out_se_ptr=5 * a),      # an output inside the records
           dict(rgba_ptr=a + 8), dict(out_hist_ptr=6 * a + 8),         # not 16-byte aligned
           dict(prev_camera=singular), dict(prev_camera=nan_cam),
           dict(prev_camera=_camera(W + 1, H)), dict(prev_camera=_camera(W, H - 1)),
           dict(prev_hist_ptr=0, prev_feat_ptr=0, prev_camera=singular)]  # a bad record even on the first frame
    for change in bad:
        with pytest.raises(api.PtmiError) as e:
            api.reproject(**dict(ok, **change))
        assert e.value.code == api.PTMI_ERR_ARG, change


def test_set_camera_null_arguments():
    lib = api.load_library()
    err = ctypes.create_string_buffer(256)
    cam = np.ascontiguousarray(np.asarray(_camera()).reshape(1))
    assert lib.ptmi_scene_set_camera(None, cam.ctypes.data_as(ctypes.c_void_p), err, len(err)) == api.PTMI_ERR_ARG
    assert err.value
    assert lib.ptmi_scene_set_camera(None, None, None, 0) == api.PTMI_ERR_ARG


def test_cli_usage_names_sequence_flags():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("--frames", "--orbit-step", "--temporal", "--max-history"):
        assert flag in text, text
    # flag misuse ends in the usage error before any device is touched
    for extra in (["--temporal"], ["--temporal", "--frames", "1"], ["--temporal", "--frames", "3", "--gpus", "2"],
                  ["--temporal", "--frames", "3", "--noise-target", "0.1"],
                  ["--temporal", "--frames", "3", "--noise-target", "0.1", "--adaptive"],
                  ["--frames", "0"], ["--max-history", "4", "--frames", "3"]):
        r = subprocess.run([PT, "--samples", "4"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage:" in r.stderr, extra
        assert "--temporal" in r.stderr or "--frames" in r.stderr
