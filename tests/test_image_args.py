"""What the image-space entry points (csrc/ptmi_image_api.cpp, checks in csrc/ptmi_image_args.h) refuse and accept,
on the CPU: every refusal returns before any device call, so the addresses are fake and never dereferenced.

Golden refusals: tests/golden/image_arg_errors.json holds calls and the (status, message) that the library gave
for them while these checks were still written out per entry point inside ptmi_api.cpp (commit 8b4c6bf; recorded
through ctypes by a throw-away script) -- NULL and zero-size arguments, every validated parameter field, outputs
equal to and overlapping inputs and each other, each aligned pointer off by 8, bad previous cameras, motion tables
without objects, and calls where two checks would fire, which pin the precedence.  A case is [entry point,
change, status, message]: the call is the entry point's baseline with `change` applied.  A refactor of the checks
must reproduce every one byte for byte.

Acceptances: tests/host_kat/image_args_kat.cpp calls the checkers of ptmi_image_args.h directly, which is the only
way to ask on a CPU what they accept.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from ptmi import api
from tests.scene_inputs import scene_inputs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_arg_errors.json")
KAT = os.path.join(ROOT, "tests", "host_kat", "build", "image_args_kat")
W, H = 36, 20

# The entry points' arguments in the C order, without the trailing (hip_stream, err, err_len).
_LOOKUP = ("rgba", "se", "feat", "prev_hist", "prev_feat", "camera", "w", "h", "params")
SIG = {
    "ptmi_select_tiles": ("tile_err", "in_tiles", "n_in", "threshold", "out_tiles", "count"),
    "ptmi_finalize_counts": ("sums", "out", "n_pixels"),
    "ptmi_finalize": ("sums", "out", "n_pixels", "samples"),
    "ptmi_fill_seeds": ("seeds", "n", "seed_stream"),
    "ptmi_combine_frames": ("parts", "n_parts", "n_pixels", "out", "samples"),
    "ptmi_error_map": ("sums", "sq", "w", "h", "se", "tile_err", "stats"),
    "ptmi_accumulate": ("dst", "src", "n"),
    "ptmi_denoise": ("rgba", "se", "feat", "w", "h", "params", "out_rgba", "out_se", "work", "work_bytes"),
    "ptmi_motion_table": ("prev_objects", "cur_objects", "n_obj", "motion"),
    "ptmi_reproject": _LOOKUP + ("out_hist", "out_rgba", "out_se"),
    "ptmi_reproject_motion": _LOOKUP + ("out_hist", "out_rgba", "out_se", "motion", "n_obj"),
    "ptmi_history_gather": _LOOKUP + ("gathered", "motion", "n_obj"),
    "ptmi_rectify": ("rgba", "se", "feat", "gathered", "w", "h", "params", "out_hist", "out_rgba", "out_se"),
    "ptmi_variance_estimate": ("rgba", "se", "feat", "prev_mom", "prev_feat", "camera", "w", "h", "params", "out_mom",
                               "out_se", "motion", "n_obj"),
}
PARAMS = {"ptmi_denoise": api.DenoiseParams, "ptmi_reproject": api.ReprojectParams,
          "ptmi_reproject_motion": api.ReprojectParams, "ptmi_history_gather": api.ReprojectParams,
          "ptmi_rectify": api.RectifyParams, "ptmi_variance_estimate": api.VarianceParams}
# The fields a call validates (ptmi_rectify takes any min_count; `reserved` is not read), the pointers it wants
# 16-byte aligned and its outputs.
VALIDATED = {"ptmi_denoise": ("iterations", "flags", "sigma_l", "sigma_d", "normal_power"),
             "ptmi_rectify": ("radius", "gamma", "max_history", "flags"),
             "ptmi_variance_estimate": tuple(n for n, _ in api.VarianceParams._fields_)}
for _fn in ("ptmi_reproject", "ptmi_reproject_motion", "ptmi_history_gather"):
    VALIDATED[_fn] = tuple(n for n, _ in api.ReprojectParams._fields_)
ALIGNED = {"ptmi_denoise": ("rgba", "feat", "out_rgba", "work"),
           "ptmi_motion_table": ("motion",),
           "ptmi_reproject": ("rgba", "feat", "prev_hist", "prev_feat", "out_hist", "out_rgba"),
           "ptmi_reproject_motion": ("rgba", "feat", "prev_hist", "prev_feat", "out_hist", "out_rgba", "motion"),
           "ptmi_history_gather": ("rgba", "feat", "prev_hist", "prev_feat", "gathered", "motion"),
           "ptmi_rectify": ("rgba", "feat", "gathered", "out_hist", "out_rgba"),
           "ptmi_variance_estimate": ("rgba", "feat", "prev_mom", "prev_feat", "out_mom", "motion")}
OUTPUTS = {"ptmi_reproject": ("out_hist", "out_rgba", "out_se"), "ptmi_reproject_motion": ("out_hist", "out_rgba", "out_se"),
           "ptmi_history_gather": ("gathered",), "ptmi_rectify": ("out_hist", "out_rgba", "out_se"),
           "ptmi_variance_estimate": ("out_mom", "out_se")}
CAMERAS = ("good", "none", "singular", "nan", "wider", "shorter", "zero_width", "pixel_zero", "pixel_nan", "half_width_nan",
           "half_height_inf")
_OBJECTS = np.zeros(16 * 1024, dtype=np.uint8)  # a refused ptmi_motion_table never reads its records


def camera(name):
    """The previous-camera record of a case, by name: the reference scene's W x H camera, or one spoiled."""
    if name == "none":
        return None
    size = {"wider": (W + 1, H), "shorter": (W, H - 1)}.get(name, (W, H))
    cam = np.array(scene_inputs("reference", *size)[3]).copy().reshape(1)
    if name == "singular":
        cam["inverse"] = np.zeros(16)
    elif name == "nan":
        cam["inverse"][0, 5] = np.nan
    elif name == "zero_width":
        cam["width"] = 0
    elif name == "pixel_zero":
        cam["pixel_size"] = 0.0
    elif name == "pixel_nan":
        cam["pixel_size"] = np.nan
    elif name == "half_width_nan":
        cam["half_width"] = np.nan
    elif name == "half_height_inf":
        cam["half_height"] = np.inf
    else:
        assert name in ("good", "wider", "shorter"), name
    return cam


def call(lib, fn, args):
    """The raw call of entry point `fn` with the case's arguments: (status, message)."""
    keep, vals = [], []
    for name in SIG[fn]:
        v = args[name]
        if name == "params":
            v = PARAMS[fn](**v) if v is not None else None
            keep.append(v)
            v = ctypes.byref(v) if v is not None else None
        elif name == "camera":
            v = camera(v)
            keep.append(v)
            v = v.ctypes.data_as(ctypes.c_void_p) if v is not None else None
        elif name in ("prev_objects", "cur_objects"):
            v = _OBJECTS.ctypes.data_as(ctypes.c_void_p) if v == "objects" else None
        vals.append(v)
    err = ctypes.create_string_buffer(512)
    status = getattr(lib, fn)(*vals, None, err, len(err))
    return status, err.value.decode()


def _table():
    doc = json.load(open(GOLDEN))
    return doc["baselines"], [dict(fn=c[0], change=c[1], status=c[2], message=c[3]) for c in doc["cases"]]


BASE, TABLE = _table()


def test_golden_refusals():
    lib = api.load_library()
    assert len(TABLE) >= 400
    bad = []
    for c in TABLE:
        got = call(lib, c["fn"], dict(BASE[c["fn"]], **c["change"]))
        if got != (c["status"], c["message"]):
            bad.append((c["fn"], c["change"], (c["status"], c["message"]), got))
    assert not bad, "%d of %d refusals differ; first: %s %s expected %s got %s" % ((len(bad), len(TABLE)) + bad[0])


def test_the_table_holds_the_cases_it_is_meant_to():
    """(so that an edit of the table cannot quietly drop a kind of case)"""
    assert set(BASE) == set(SIG) and {c["fn"] for c in TABLE} == set(SIG)
    assert all(c["status"] == api.PTMI_ERR_ARG and c["message"] for c in TABLE)
    by_fn = {fn: [c for c in TABLE if c["fn"] == fn] for fn in SIG}
    alone = {fn: [c for c in cs if len(c["change"]) == 1] for fn, cs in by_fn.items()}
    for fn, names in SIG.items():  # every pointer NULL and every size 0 that the call minds
        base = BASE[fn]
        assert set(base) == set(names), fn
    for fn, fields in VALIDATED.items():  # every validated parameter field, alone, named by the parameter message
        seen = {k for c in alone[fn] if c["change"].get("params") for k in c["change"]["params"]
                if len(c["change"]["params"]) == 1 and "parameters" in c["message"]}
        assert seen >= set(fields), (fn, set(fields) - seen)
    for fn, names in ALIGNED.items():  # each aligned pointer 8 past its baseline, alone
        for n in names:
            assert any(c["change"] == {n: BASE[fn][n] + 8} or
                       (n == "motion" and not BASE[fn][n] and c["change"].get(n, 0) % 16 == 8 and len(c["change"]) == 2)
                       for c in by_fn[fn]), (fn, n)
    for fn, outs in OUTPUTS.items():  # per output: on an input's address (equality) and across one's edge (overlap)
        ins = [n for n in SIG[fn] if isinstance(BASE[fn][n], int) and BASE[fn][n] >= 0x100000 and n not in outs]
        for o in outs:
            moved = [c["change"][o] for c in alone[fn] if o in c["change"] and "overlap" in c["message"]]
            assert any(v in [BASE[fn][i] for i in ins] for v in moved), (fn, o, "equality")
            assert any(v % 8 == 0 and v not in [BASE[fn][n] for n in SIG[fn] if isinstance(BASE[fn][n], int)] for v in moved), \
                (fn, o, "overlap")
        if len(outs) > 1:  # an output inside another output
            assert any(any(0 < c["change"][o] - BASE[fn][q] < 4096 for q in outs if q != o) for c in alone[fn]
                       for o in outs if o in c["change"]), fn
    assert any(c["change"] == {"out_rgba": BASE["ptmi_denoise"]["rgba"]} for c in by_fn["ptmi_denoise"])
    for fn in ("ptmi_reproject", "ptmi_reproject_motion", "ptmi_history_gather", "ptmi_variance_estimate"):
        assert {c["change"]["camera"] for c in alone[fn] if "camera" in c["change"]} >= set(CAMERAS) - {"good"}, fn
        assert any("bad camera size" in c["message"] for c in by_fn[fn])
    # motion table / object-count mismatch, both ways, and too many objects
    for fn in ("ptmi_history_gather", "ptmi_variance_estimate"):
        given = {(bool(a["motion"]), a["n_obj"]) for a in (dict(BASE[fn], **c["change"]) for c in by_fn[fn])
                 if True}
        assert {(True, 0), (False, 3), (True, 17)} <= given, fn
    moved = [dict(BASE["ptmi_reproject_motion"], **c["change"]) for c in by_fn["ptmi_reproject_motion"]]
    assert {(bool(a["motion"]), a["n_obj"]) for a in moved} >= {(False, 8), (True, 0), (True, 17)}
    # frame sizes past each limit: a side, and the pixel count
    for fn in PARAMS:
        sizes = {(a["w"], a["h"]) for a in (dict(BASE[fn], **c["change"]) for c in by_fn[fn])}
        assert sizes >= {(0, H), (W, 0), (65537, 1), (1, 65537), (65536, 32769)}, fn
    # two checks at once: the size or a NULL with a parameter, a parameter with an overlap, an overlap with a camera
    for fn in PARAMS:
        both = [c["change"] for c in by_fn[fn] if len(c["change"]) >= 2]
        assert any("params" in ch and ("w" in ch or "h" in ch) for ch in both), fn
        if fn != "ptmi_denoise":
            assert any("params" in ch and set(ch) & set(OUTPUTS[fn]) for ch in both), fn
        if "camera" in SIG[fn]:
            assert any("camera" in ch and set(ch) & set(OUTPUTS[fn]) for ch in both), fn


def test_checkers_accept_what_the_entry_points_did():
    if not os.path.exists(KAT):
        pytest.fail("tests/host_kat not built (run __graft_entry__.build())")
    r = subprocess.run([KAT], capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert len(lines) >= 60 and all(l.startswith("PASS") for l in lines), r.stdout
    assert r.returncode == 0
