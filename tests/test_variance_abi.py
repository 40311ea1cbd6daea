"""The variance-estimation boundary on CPU (no GPU calls): include/ptmi.h declares ptmi_variance_estimate,
libptmi.so exports it, the Python binding's parameter record has the header's layout, every PTMI_ERR_ARG case
is refused before any device call (the pointers below are never dereferenced), and the CLI refuses
--estimate-variance without --temporal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ptmi import api, temporal
from tests.scene_inputs import scene_inputs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")
W, H = 36, 20
FIELDS = [("max_history", 0), ("min_temporal", 4), ("radius", 8), ("min_count", 12), ("flags", 16), ("normal_cos", 24),
          ("plane_dist", 32), ("min_weight", 40), ("window_normal_cos", 48)]


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "ptmi_variance_estimate" in set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert "ptmi_variance_estimate" in api.EXPORTS
    assert re.search(r"#define\s+PTMI_MOMENT_DOUBLES\s+8\b", src)
    assert api.MOMENT_DOUBLES == 8 and temporal.MOMENT_DOUBLES == 8
    # the struct's fields, in the header's order
    body = re.search(r"typedef struct ptmi_variance_params \{(.*?)\} ptmi_variance_params;", src, re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in FIELDS]
    # the points the header must state
    assert "variance_reference" in text and "not rectified" in text


def test_library_exports_the_entry_point():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "ptmi_variance_estimate" in {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_params_layout_and_defaults():
    """The ctypes record is the header's struct: five uint32, four bytes of padding, four doubles."""
    assert ctypes.sizeof(api.VarianceParams) == 56
    assert [(n, getattr(api.VarianceParams, n).offset) for n, _ in api.VarianceParams._fields_] == FIELDS
    p = api.VarianceParams()
    got = {n: getattr(p, n) for n, _ in FIELDS}
    assert got == dict(max_history=32, min_temporal=4, radius=3, min_count=9, flags=0, normal_cos=0.9, plane_dist=0.02,
                       min_weight=0.05, window_normal_cos=0.9)
    assert temporal.VARIANCE_DEFAULTS == got and temporal.variance_params_dict(p) == got
    assert api.variance_params({"radius": 2}).radius == 2 and api.variance_params(None) is None
    for bad in (dict(max_history=0), dict(max_history=65537), dict(min_temporal=1), dict(min_temporal=65537),
                dict(radius=0), dict(radius=5), dict(min_count=1), dict(flags=1), dict(normal_cos=-1.0),
                dict(plane_dist=float("nan")), dict(min_weight=float("inf")), dict(window_normal_cos=-0.5)):
        with pytest.raises(ValueError):
            temporal.variance_params_dict(bad)


def _camera(w=W, h=H):
    return scene_inputs("reference", w, h)[3]


def test_argument_errors_need_no_device():
    """Fake, 16-byte-aligned addresses: an accepted call would fault, a refused one never touches them."""
    a = 0x100000  # (further apart than the largest buffer, 36 x 20 x 96 bytes)
    ok = dict(rgba_ptr=a, se_ptr=2 * a, feat_ptr=3 * a, prev_mom_ptr=4 * a, prev_feat_ptr=5 * a, prev_camera=_camera(),
              w=W, h=H, out_mom_ptr=6 * a, out_se_ptr=7 * a, motion_ptr=8 * a, n_obj=3)
    singular = _camera().copy()
    singular["inverse"] = np.zeros(16)
    nan_cam = _camera().copy()
    nan_cam["inverse"][5] = np.nan
    bad = [dict(rgba_ptr=0), dict(feat_ptr=0), dict(out_mom_ptr=0), dict(out_se_ptr=0),
           dict(prev_feat_ptr=0), dict(prev_camera=None),             # required once there is a history
           dict(w=0), dict(h=0),
           dict(params=dict(max_history=0)), dict(params=dict(max_history=65537)),
           dict(params=dict(min_temporal=1)), dict(params=dict(min_temporal=0)), dict(params=dict(min_temporal=65537)),
           dict(params=dict(radius=0)), dict(params=dict(radius=5)),
           dict(params=dict(min_count=1)), dict(params=dict(min_count=0)), dict(params=dict(flags=1)),
           dict(params=dict(normal_cos=-0.1)), dict(params=dict(normal_cos=float("nan"))),
           dict(params=dict(plane_dist=-1.0)), dict(params=dict(plane_dist=float("inf"))),
           dict(params=dict(min_weight=-0.5)), dict(params=dict(min_weight=float("nan"))),
           dict(params=dict(window_normal_cos=-0.5)), dict(params=dict(window_normal_cos=float("inf"))),
           dict(out_mom_ptr=4 * a),                                    # aliased moments
           dict(out_mom_ptr=4 * a + 16), dict(out_mom_ptr=4 * a - 16),  # ... overlapping, not equal
           dict(out_mom_ptr=4 * a + W * H * 64 - 16),                  # ... by its last 16 bytes
           dict(out_se_ptr=2 * a), dict(out_se_ptr=a + 8),             # no in-place standard error
           dict(out_se_ptr=6 * a + 8),                                 # an output inside the other output
           dict(out_mom_ptr=3 * a + 96), dict(out_se_ptr=5 * a),       # an output inside the records
           dict(out_mom_ptr=8 * a), dict(out_se_ptr=8 * a + 64),       # ... inside the motion table
           dict(rgba_ptr=a + 8), dict(feat_ptr=3 * a + 8), dict(prev_mom_ptr=4 * a + 8), dict(prev_feat_ptr=5 * a + 8),
           dict(out_mom_ptr=6 * a + 8), dict(motion_ptr=8 * a + 8),    # not 16-byte aligned
           dict(prev_camera=singular), dict(prev_camera=nan_cam),
           dict(prev_camera=_camera(W + 1, H)), dict(prev_camera=_camera(W, H - 1)),
           dict(prev_mom_ptr=0, prev_feat_ptr=0, prev_camera=singular),  # a bad record even on the first frame
           dict(motion_ptr=0), dict(n_obj=0),                          # a table without objects, objects without a table
           dict(n_obj=17)]
    for change in bad:
        with pytest.raises(api.PtmiError) as e:
            api.variance_estimate(**dict(ok, **change))
        assert e.value.code == api.PTMI_ERR_ARG, change
    # the raw call with every pointer NULL, error buffer included
    assert api.load_library().ptmi_variance_estimate(None, None, None, None, None, None, W, H, None, None, None, None, 0,
                                                     None, None, 0) == api.PTMI_ERR_ARG


def test_cli_names_the_flags_and_needs_temporal():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--help"], capture_output=True, text=True, timeout=60)
    for flag in ("--estimate-variance", "--var-min-history", "--var-radius"):
        assert flag in r.stdout + r.stderr
    # flag misuse ends in the usage error before any device is touched
    for extra, word in ((["--estimate-variance"], "--temporal"),
                        (["--estimate-variance", "--frames", "3"], "--temporal"),
                        (["--var-radius", "2", "--frames", "3", "--temporal"], "--estimate-variance"),
                        (["--var-min-history", "3", "--frames", "3", "--temporal"], "--estimate-variance"),
                        (["--estimate-variance", "--var-radius", "5", "--frames", "3", "--temporal"], "--var-radius"),
                        (["--estimate-variance", "--var-min-history", "1", "--frames", "3", "--temporal"],
                         "--var-min-history")):
        r = subprocess.run([PT, "--samples", "4"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage:" in r.stderr and word in r.stderr.split("usage:")[0], extra
    # without the flag 1 spp is still refused for --temporal
    r = subprocess.run([PT, "--samples", "1", "--frames", "3", "--temporal"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--samples >= 2" in r.stderr
