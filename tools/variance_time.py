"""DIAGNOSTIC: the measurements of profiles/variance/SUMMARY.md -- ptmi_variance_estimate at 1280 x 960 by HIP
events on a first frame (every pixel walks the window), with a short history (the third frame: the lookup and the
window) and with a full history (the window is skipped), beside ptmi_history_gather and ptmi_rectify timed in the
same run; reference scene (C2) and teapot (C4), 4 spp, a 1.5-degree-per-frame orbit.
    python tools/variance_time.py [reference] [teapot]"""
import os
import sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-ocl_amd"))
sys.path.insert(0, ROOT)
from ptmi import api, temporal
from tests.scene_inputs import scene_inputs


def timings(scene, w=1280, h=960, spp=4, frames=6):
    objs, tris, grps, cam = scene_inputs(scene, w, h)
    cams = [temporal.orbit_camera(cam, 1.5 * k) for k in range(frames)]
    sc = api.Scene(0, objs, tris, grps, cam)
    n = w * h
    kw = dict(dtype=torch.float64, device="cuda")
    keep = []
    for f in temporal.render_sequence(sc, cams, spp, 300, temporal=True, variance="estimated",
                                      chunks=2 if tris.size else 0):
        torch.cuda.synchronize()
        keep.append({k: v.clone() for k, v in f.items()})
    sc.close()
    mom, se_est, gathered, hist = torch.empty(n * 8, **kw), torch.empty(n, **kw), torch.empty(n * 8, **kw), \
        torch.empty(n * 8, **kw)
    acc, acc_se = torch.empty(n * 4, **kw), torch.empty(n, **kw)

    def frame(k):
        return keep[k]["image"].data_ptr(), keep[k]["se"].data_ptr(), keep[k]["feat"].data_ptr()

    def variance(k, **params):
        prev = keep[k - 1] if k else None
        return lambda: api.variance_estimate(*frame(k), prev["moments"].data_ptr() if prev else 0,
                                             prev["feat"].data_ptr() if prev else 0, cams[k - 1] if k else None, w, h,
                                             mom.data_ptr(), se_est.data_ptr(), params=params or None)
    last = frames - 1
    calls = {"variance first frame": variance(0), "variance first frame r=1": variance(0, radius=1),
             "variance first frame r=4": variance(0, radius=4), "variance third frame": variance(2),
             "variance full history": variance(last),
             "history_gather": lambda: api.history_gather(*frame(last), keep[last - 1]["hist"].data_ptr(),
                                                          keep[last - 1]["feat"].data_ptr(), cams[last - 1], w, h,
                                                          gathered.data_ptr()),
             "rectify": lambda: api.rectify(*frame(last), gathered.data_ptr(), w, h, hist.data_ptr(),
                                            out_rgba_ptr=acc.data_ptr(), out_se_ptr=acc_se.data_ptr())}
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        extra = ""
        if name.startswith("variance"):
            src = mom.view(n, 8)[:, 5]
            extra = "  sources temporal %.4f spatial %.4f fallback %.4f" % tuple(
                float((src == v).double().mean()) for v in (1.0, 2.0, 3.0))
        print("TIMING %s %dx%d %-26s median %.4f ms  min %.4f  max %.4f (30 runs)%s" %
              (scene, w, h, name, ts[15], ts[0], ts[-1], extra), flush=True)


if __name__ == "__main__":
    for scene in (sys.argv[1:] or ["reference", "teapot"]):
        timings(scene)
