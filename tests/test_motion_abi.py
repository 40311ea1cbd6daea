"""The object-update / motion-reprojection boundary on CPU (no GPU calls): include/ptmi.h declares
ptmi_scene_set_objects, ptmi_motion_table and ptmi_reproject_motion, libptmi.so exports them, and every
PTMI_ERR_ARG case of the two motion calls is refused before any device call (the device pointers below
are fake and never dereferenced)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ptmi import api, temporal
from tests.scene_inputs import scene_inputs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ptmi_scene_set_objects", "ptmi_motion_table", "ptmi_reproject_motion")
W, H = 36, 20


def test_header_declares_motion_entry_points():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert set(NEW) <= set(api.EXPORTS)
    assert re.search(r"#define\s+PTMI_MOTION_DOUBLES\s+24\b", src)
    assert api.MOTION_DOUBLES == 24 and temporal.MOTION_DOUBLES == 24
    assert text.count("HOST-BLOCKING") >= 2  # set_objects states it as set_camera does


def test_library_exports_motion_entry_points():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def _objects():
    return scene_inputs("reference", W, H)[0]


def test_motion_table_argument_errors_need_no_device():
    objs = _objects()
    a = 0x100000
    ok = dict(prev_objects=objs, cur_objects=objs, motion_ptr=a, n_obj=len(objs))
    for change in (dict(prev_objects=None), dict(cur_objects=None), dict(motion_ptr=0), dict(n_obj=0), dict(n_obj=17),
                   dict(motion_ptr=a + 8)):
        with pytest.raises(api.PtmiError) as e:
            api.motion_table(**dict(ok, **change))
        assert e.value.code == api.PTMI_ERR_ARG, change


def test_reproject_motion_argument_errors_need_no_device():
    """ptmi_reproject's refusals (tests/test_temporal_abi.py) and the motion table's, on fake addresses."""
    a = 0x100000  # (further apart than the largest buffer, 36 x 20 x 96 bytes)
    cam = scene_inputs("reference", W, H)[3]
    ok = dict(rgba_ptr=a, se_ptr=2 * a, feat_ptr=3 * a, prev_hist_ptr=4 * a, prev_feat_ptr=5 * a, prev_camera=cam,
              w=W, h=H, out_hist_ptr=6 * a, out_rgba_ptr=7 * a, out_se_ptr=8 * a, motion_ptr=9 * a, n_obj=8)
    singular = cam.copy()
    singular["inverse"] = np.zeros(16)
    nan_cam = cam.copy()
    nan_cam["inverse"][5] = np.nan
    bad = [dict(motion_ptr=0), dict(n_obj=0), dict(n_obj=17), dict(motion_ptr=9 * a + 8),   # the table itself
           dict(out_hist_ptr=9 * a), dict(out_rgba_ptr=9 * a + 16),                         # an output on the table
           dict(out_se_ptr=9 * a + 8 * 24 * 8 - 8), dict(out_hist_ptr=9 * a - 16),          # ... by its last / first bytes
           dict(rgba_ptr=0), dict(se_ptr=0), dict(feat_ptr=0), dict(out_hist_ptr=0),
           dict(prev_feat_ptr=0), dict(prev_camera=None), dict(w=0), dict(h=0),
           dict(params=dict(max_history=0)), dict(params=dict(max_history=65537)), dict(params=dict(flags=1)),
           dict(params=dict(normal_cos=-0.1)), dict(params=dict(normal_cos=float("nan"))),
           dict(params=dict(plane_dist=-1.0)), dict(params=dict(plane_dist=float("inf"))),
           dict(params=dict(min_weight=-0.5)), dict(params=dict(min_weight=float("nan"))),
           dict(out_hist_ptr=4 * a), dict(out_hist_ptr=4 * a + 16), dict(out_hist_ptr=4 * a - 16),
           dict(out_hist_ptr=4 * a + W * H * 64 - 16), dict(out_rgba_ptr=a), dict(out_se_ptr=2 * a),
           dict(out_rgba_ptr=6 * a + 32), dict(out_se_ptr=7 * a + 8), dict(out_hist_ptr=3 * a + 96),
           dict(out_se_ptr=5 * a), dict(rgba_ptr=a + 8), dict(out_hist_ptr=6 * a + 8),
           dict(prev_camera=singular), dict(prev_camera=nan_cam),
           dict(prev_camera=scene_inputs("reference", W + 1, H)[3]), dict(prev_camera=scene_inputs("reference", W, H - 1)[3])]
    for change in bad:
        with pytest.raises(api.PtmiError) as e:
            api.reproject_motion(**dict(ok, **change))
        assert e.value.code == api.PTMI_ERR_ARG, change


def test_set_objects_null_arguments():
    lib = api.load_library()
    err = ctypes.create_string_buffer(256)
    objs = np.ascontiguousarray(_objects())
    assert lib.ptmi_scene_set_objects(None, objs.ctypes.data_as(ctypes.c_void_p), len(objs), err, len(err)) == \
        api.PTMI_ERR_ARG
    assert err.value
    assert lib.ptmi_scene_set_objects(None, None, 0, None, 0) == api.PTMI_ERR_ARG
