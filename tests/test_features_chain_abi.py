"""The specular-chain feature pass's boundary on CPU (no GPU calls): include/ptmi.h declares
ptmi_scene_features_chain, libptmi.so exports it, every PTMI_ERR_ARG case is refused before any device
call (the pointers below are never dereferenced), Scene.features keeps today's call as its default, the
`guides` keyword is where the frame loops take it, and the CLI refuses --guides where it does not apply."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from ptmi import api, denoise, error, temporal

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ptmi_scene_features_chain",)
PT = os.path.join(ROOT, "pathtracer-ocl_amd", "build", "pt")


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z_]+)\s*\(", src))
    assert set(NEW) <= declared
    assert set(NEW) <= set(api.EXPORTS)
    m = re.search(r"int\s+ptmi_scene_features_chain\s*\(([^)]*)\)", src)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["s", "feat_dev", "max_chain", "reflect_min", "hip_stream", "err", "err_len"]


def test_library_exports_the_entry_point():
    if not os.path.exists(api.LIB_PATH):
        pytest.fail("libptmi.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported


def test_argument_errors_need_no_device():
    """Fake addresses: an accepted call would fault on them, a refused one never touches them."""
    lib = api.load_library()
    scene, feat = 0x100000, 0x200000
    ok = dict(s=scene, feat=feat, max_chain=8, reflect_min=0.5)
    bad = [dict(s=None), dict(feat=None), dict(feat=feat + 8), dict(max_chain=0), dict(max_chain=17),
           dict(max_chain=0xFFFFFFFF), dict(reflect_min=0.0), dict(reflect_min=-0.5), dict(reflect_min=1.0 + 2.0 ** -52),
           dict(reflect_min=float("nan")), dict(reflect_min=float("inf"))]
    for change in bad:
        a = dict(ok, **change)
        err = ctypes.create_string_buffer(256)
        rc = lib.ptmi_scene_features_chain(ctypes.c_void_p(a["s"]), ctypes.c_void_p(a["feat"]), a["max_chain"],
                                           a["reflect_min"], None, err, len(err))
        assert rc == api.PTMI_ERR_ARG, change
        assert err.value, change


def test_python_keywords_default_to_the_first_hit():
    sig = inspect.signature(api.Scene.features)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == \
        [("feat_ptr", inspect.Parameter.empty), ("stream", 0), ("chain", False), ("max_chain", 8), ("reflect_min", 0.5)]
    for fn in (denoise.render_denoised, denoise.denoise_frame, temporal.render_sequence, error.render_to_noise,
               error.render_adaptive):
        assert inspect.signature(fn).parameters["guides"].default == "first", fn.__name__
    assert denoise.GUIDES == ("first", "specular")


def test_bad_guides_and_moving_objects_are_refused():
    """Before any device call: the scene is never touched."""
    with pytest.raises(ValueError, match="objects"):
        next(temporal.render_sequence(None, [], 2, 0, objects=[], guides="specular"))
    with pytest.raises(ValueError, match="guides"):
        next(temporal.render_sequence(None, [], 2, 0, guides="second"))
    with pytest.raises(ValueError, match="guides"):
        denoise.render_denoised(None, 2, 0, guides="second")
    with pytest.raises(ValueError, match="guides"):
        denoise.denoise_frame(None, None, None, guides="")


def test_cli_usage_names_the_guides_flags():
    if not os.path.exists(PT):
        pytest.fail("pt CLI not built")
    r = subprocess.run([PT, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("--guides", "--max-chain"):
        assert flag in text, text
    # flag misuse ends in the usage error before any device is touched
    seq = ["--frames", "3", "--samples", "2", "--temporal"]
    for args, word in ((["--denoise", "--guides", "second"], "--guides"),
                       (["--guides", "specular"], "--guides"),
                       (["--denoise", "--max-chain", "4"], "--max-chain"),
                       (["--denoise", "--guides", "specular", "--max-chain", "0"], "--max-chain"),
                       (["--denoise", "--guides", "specular", "--max-chain", "17"], "--max-chain"),
                       (seq + ["--guides", "specular", "--move-object", "6", "--move-step", "0.01,0,0"],
                        "--move-object")):
        r = subprocess.run([PT] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr.splitlines()[0] and "usage:" in r.stderr, (args, r.stderr)
