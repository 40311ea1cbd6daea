"""The history-rectification boundary on CPU (no GPU calls): include/ptmi.h declares ptmi_history_gather and
ptmi_rectify, libptmi.so exports them, the Python binding's parameter record has the header's layout, and
every PTMI_ERR_ARG case of both calls is refused before any device call (the pointers below are never
dereferenced), and the CLI refuses --rectify and --emission-step where they do not apply."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ptmi import api, temporal
from tests.scene_inputs import scene_inputs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ptmi_history_gather", "ptmi_rectify")
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")
W, H = 36, 20


def test_header_declares_rectify_entry_points():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert set(NEW) <= set(api.EXPORTS)
    assert re.search(r"typedef\s+struct\s+ptmi_rectify_params\s*\{\s*uint32_t\s+radius;\s*uint32_t\s+min_count;\s*"
                     r"double\s+gamma;\s*uint32_t\s+max_history;\s*uint32_t\s+flags;\s*\}", src)
    # the limits the header must state, and no promise of a lag any more
    for phrase in ("window MEAN", "min_count", "independent"):
        assert phrase in text, phrase
    assert "lag by the history length" not in text and "lags by the history" not in text


def test_library_exports_rectify_entry_points():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def test_params_layout_and_defaults():
    """The ctypes record is the header's struct: 4 + 4 + 8 + 4 + 4 bytes; its defaults are the documented ones."""
    assert ctypes.sizeof(api.RectifyParams) == 24
    assert [(n, getattr(api.RectifyParams, n).offset) for n, _ in api.RectifyParams._fields_] == \
        [("radius", 0), ("min_count", 4), ("gamma", 8), ("max_history", 16), ("flags", 20)]
    p = api.RectifyParams()
    assert (p.radius, p.min_count, p.gamma, p.max_history, p.flags) == (3, 9, 3.0, 32, 0)
    assert temporal.RECTIFY_DEFAULTS == dict(radius=3, min_count=9, gamma=3.0, max_history=32, flags=0)
    assert api.rectify_params({"radius": 2}).radius == 2 and api.rectify_params(None) is None


def _camera(w=W, h=H):
    return scene_inputs("reference", w, h)[3]


def _refused(call, ok, bad):
    for change in bad:
        with pytest.raises(api.PtmiError) as e:
            call(**dict(ok, **change))
        assert e.value.code == api.PTMI_ERR_ARG, change


def test_history_gather_argument_errors_need_no_device():
    """Fake, 16-byte-aligned addresses: an accepted call would fault, a refused one never touches them."""
    a = 0x100000  # (further apart than the largest buffer, 36 x 20 x 96 bytes)
    ok = dict(rgba_ptr=a, se_ptr=2 * a, feat_ptr=3 * a, prev_hist_ptr=4 * a, prev_feat_ptr=5 * a, prev_camera=_camera(),
              w=W, h=H, gathered_ptr=6 * a)
    singular = _camera().copy()
    singular["inverse"] = np.zeros(16)
    nan_cam = _camera().copy()
    nan_cam["inverse"][5] = np.nan
    bad = [dict(rgba_ptr=0), dict(se_ptr=0), dict(feat_ptr=0), dict(gathered_ptr=0),
           dict(prev_feat_ptr=0), dict(prev_camera=None),             # required once there is a history
           dict(w=0), dict(h=0),
           dict(params=dict(max_history=0)), dict(params=dict(max_history=65537)), dict(params=dict(flags=1)),
           dict(params=dict(normal_cos=-0.1)), dict(params=dict(normal_cos=float("nan"))),
           dict(params=dict(plane_dist=-1.0)), dict(params=dict(plane_dist=float("inf"))),
           dict(params=dict(min_weight=-0.5)), dict(params=dict(min_weight=float("nan"))),
           dict(gathered_ptr=4 * a),                                   # aliased history
           dict(gathered_ptr=4 * a + 16), dict(gathered_ptr=4 * a - 16),  # ... overlapping, not equal
           dict(gathered_ptr=4 * a + W * H * 64 - 16),                 # ... by its last 16 bytes
           dict(gathered_ptr=a), dict(gathered_ptr=2 * a),             # the output inside the frame or its error map
           dict(gathered_ptr=3 * a + 96), dict(gathered_ptr=5 * a),    # ... inside the records
           dict(rgba_ptr=a + 8), dict(gathered_ptr=6 * a + 8),         # not 16-byte aligned
           dict(prev_camera=singular), dict(prev_camera=nan_cam),
           dict(prev_camera=_camera(W + 1, H)), dict(prev_camera=_camera(W, H - 1)),
           dict(prev_hist_ptr=0, prev_feat_ptr=0, prev_camera=singular),  # a bad record even on the first frame
           # the motion table and its length go together; 1..16 objects; aligned; not the output
           dict(motion_ptr=7 * a), dict(n_obj=3), dict(motion_ptr=7 * a, n_obj=17),
           dict(motion_ptr=7 * a + 8, n_obj=3), dict(motion_ptr=6 * a + 64, n_obj=3)]
    _refused(api.history_gather, ok, bad)


def test_rectify_argument_errors_need_no_device():
    a = 0x100000
    ok = dict(rgba_ptr=a, se_ptr=2 * a, feat_ptr=3 * a, gathered_ptr=4 * a, w=W, h=H, out_hist_ptr=6 * a,
              out_rgba_ptr=7 * a, out_se_ptr=8 * a)
    bad = [dict(rgba_ptr=0), dict(se_ptr=0), dict(feat_ptr=0), dict(gathered_ptr=0), dict(out_hist_ptr=0),
           dict(w=0), dict(h=0),
           dict(params=dict(radius=0)), dict(params=dict(radius=5)),
           dict(params=dict(gamma=-0.1)), dict(params=dict(gamma=float("nan"))), dict(params=dict(gamma=float("inf"))),
           dict(params=dict(max_history=0)), dict(params=dict(max_history=65537)), dict(params=dict(flags=1)),
           dict(out_hist_ptr=4 * a),                                   # in place on the gathered record
           dict(out_hist_ptr=4 * a + 16), dict(out_hist_ptr=4 * a - 16),  # ... overlapping, not equal
           dict(out_hist_ptr=4 * a + W * H * 64 - 16),                 # ... by its last 16 bytes
           dict(out_rgba_ptr=4 * a + 32), dict(out_se_ptr=4 * a + 8),  # another output inside the gathered record
           dict(out_rgba_ptr=a), dict(out_se_ptr=2 * a),               # no in-place outputs
           dict(out_rgba_ptr=6 * a + 32), dict(out_se_ptr=7 * a + 8),  # an output inside another output
           dict(out_hist_ptr=3 * a + 96), dict(out_se_ptr=3 * a),      # an output inside the records
           dict(rgba_ptr=a + 8), dict(gathered_ptr=4 * a + 8), dict(out_hist_ptr=6 * a + 8),  # not 16-byte aligned
           dict(feat_ptr=3 * a + 8), dict(out_rgba_ptr=7 * a + 8)]
    _refused(api.rectify, ok, bad)


def test_cli_usage_names_rectify_flags():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("--rectify", "--rectify-gamma", "--rectify-radius", "--emission-step"):
        assert flag in text, text
    # flag misuse ends in the usage error before any device is touched
    seq = ["--frames", "4", "--temporal"]
    for extra in (["--rectify"], ["--rectify", "--frames", "4"], ["--rectify", "--temporal"],
                  seq + ["--rectify-gamma", "2"], seq + ["--rectify-radius", "2"],
                  seq + ["--rectify", "--rectify-gamma", "-1"], seq + ["--rectify", "--rectify-gamma", "nan"],
                  seq + ["--rectify", "--rectify-radius", "0"], seq + ["--rectify", "--rectify-radius", "5"],
                  ["--emission-step", "0.5"], ["--frames", "1", "--emission-step", "0.5"],
                  seq + ["--emission-step", "-1"], seq + ["--emission-step", "inf"]):
        r = subprocess.run([PT, "--samples", "4"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage:" in r.stderr, extra
        assert "--rectify" in r.stderr.split("usage:")[0] or "--emission-step" in r.stderr.split("usage:")[0] or \
            "--temporal" in r.stderr.split("usage:")[0], (extra, r.stderr)
