"""DIAGNOSTIC: the cost of an object update and of the motion-aware reprojection on one GPU.
    python tools/motion_time.py [--width 1280 --height 960 --runs 5]
Prints, per scene (reference, teapot): the host wall-clock time of Scene.set_objects (one object
translated, the device idle before each call) beside that of creating the scene; and for the reference
scene the device time of ptmi_reproject_motion beside ptmi_reproject on the same two 16-spp frames (one
ball moved between them, both optional outputs written), by events on the stream after one warm-up."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-ocl_amd"))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from ptmi import api, geom, temporal
    from tests.scene_inputs import scene_inputs
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    w, h = a.width, a.height
    for scene, index in (("reference", 7), ("teapot", 6)):
        objs, tris, grps, cam = scene_inputs(scene, w, h)
        moved = [temporal.move_object(objs, index, geom.translate(0.01 * k, 0.0, 0.0)) for k in range(a.runs + 1)]
        t_create, t_set = [], []
        for k in range(a.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc = api.Scene(0, objs, tris, grps, cam)
            t_create.append((time.perf_counter() - t0) * 1e3)
            sc.close()
        sc = api.Scene(0, objs, tris, grps, cam)
        for k in range(a.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.set_objects(moved[k])
            t_set.append((time.perf_counter() - t0) * 1e3)
        sc.close()
        print("%s %dx%d: set_objects %.3f-%.3f ms, create %.3f-%.3f ms (host, %d calls after one warm-up)" %
              (scene, w, h, min(t_set[1:]), max(t_set[1:]), min(t_create[1:]), max(t_create[1:]), a.runs))
    objs, tris, grps, cam = scene_inputs("reference", w, h)
    objs_b = temporal.move_object(objs, 7, geom.translate(0.05, 0.0, 0.0))
    sc = api.Scene(0, objs, tris, grps, cam)
    keep = []
    for f in temporal.render_sequence(sc, [cam, cam], 16, 300, temporal=False, objects=[objs, objs_b]):
        torch.cuda.synchronize()
        keep.append({k: f[k].clone() for k in ("image", "se", "feat")})
    sc.close()
    n = w * h
    kw = dict(dtype=torch.float64, device="cuda")
    hist0, hist1, acc, acc_se = torch.empty(n * 8, **kw), torch.empty(n * 8, **kw), torch.empty(n * 4, **kw), torch.empty(n, **kw)
    table = torch.empty(api.MOTION_DOUBLES * len(objs), **kw)
    api.motion_table(objs, objs_b, table.data_ptr())
    f0, f1 = keep
    api.reproject(f0["image"].data_ptr(), f0["se"].data_ptr(), f0["feat"].data_ptr(), 0, 0, None, w, h, hist0.data_ptr())

    def call(motion):
        args = (f1["image"].data_ptr(), f1["se"].data_ptr(), f1["feat"].data_ptr(), hist0.data_ptr(), f0["feat"].data_ptr(),
                cam, w, h, hist1.data_ptr())
        kwargs = dict(out_rgba_ptr=acc.data_ptr(), out_se_ptr=acc_se.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        if motion:
            api.reproject_motion(*args, table.data_ptr(), len(objs), **kwargs)
        else:
            api.reproject(*args, **kwargs)

    for motion in (False, True, False, True):
        call(motion)
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(motion)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        blended = float((hist1.view(-1, 8)[:, 4] > 1.0).double().mean())
        print("%s %dx%d: %.3f-%.3f ms (%d runs), %.1f %% of the pixels blended" %
              ("ptmi_reproject_motion" if motion else "ptmi_reproject       ", w, h, min(ms), max(ms), a.runs, 100 * blended))


if __name__ == "__main__":
    main()
