"""DIAGNOSTIC: the measurements of profiles/rectify/SUMMARY.md -- the image passes at 1280 x 960 by HIP events
(reproject, history_gather, rectify at radius 1..4, denoise), and the moving-ball sequence of
tests/test_gpu_motion_sequence.py with and without rectification over the pixels whose light changed.
    python tools/rectify_time.py [--ball-only]"""
import os
import sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-ocl_amd"))
sys.path.insert(0, ROOT)
from ptmi import api, geom, temporal
from tests.scene_inputs import scene_inputs


def timings():
    w, h, spp = 1280, 960, 8
    objs, tris, grps, cam = scene_inputs("reference", w, h)
    cams = [temporal.orbit_camera(cam, 1.5 * k) for k in range(3)]
    sc = api.Scene(0, objs, tris, grps, cam)
    n = w * h
    kw = dict(dtype=torch.float64, device="cuda")
    keep = []
    for f in temporal.render_sequence(sc, cams, spp, 300, temporal=True):
        torch.cuda.synchronize()
        keep.append({k: v.clone() for k, v in f.items()})
    prev, cur = keep[1], keep[2]
    gathered, hist, acc, acc_se, dn = torch.empty(n * 8, **kw), torch.empty(n * 8, **kw), torch.empty(n * 4, **kw), \
        torch.empty(n, **kw), torch.empty(n * 4, **kw)
    work = torch.empty(api.denoise_work_bytes(w, h) // 8, **kw)
    a = (cur["image"].data_ptr(), cur["se"].data_ptr(), cur["feat"].data_ptr())
    calls = {
        "reproject": lambda: api.reproject(*a, prev["hist"].data_ptr(), prev["feat"].data_ptr(), cams[1], w, h, hist.data_ptr(),
                                           out_rgba_ptr=acc.data_ptr(), out_se_ptr=acc_se.data_ptr()),
        "history_gather": lambda: api.history_gather(*a, prev["hist"].data_ptr(), prev["feat"].data_ptr(), cams[1], w, h,
                                                     gathered.data_ptr()),
    }
    for r in (1, 2, 3, 4):
        calls["rectify r=%d" % r] = lambda r=r: api.rectify(*a, gathered.data_ptr(), w, h, hist.data_ptr(),
                                                            out_rgba_ptr=acc.data_ptr(), out_se_ptr=acc_se.data_ptr(),
                                                            params=dict(radius=r))
    calls["denoise"] = lambda: api.denoise(acc.data_ptr(), acc_se.data_ptr(), cur["feat"].data_ptr(), w, h, dn.data_ptr(),
                                           work=work)
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
        print("TIMING %dx%d %-16s median %.4f ms  min %.4f  max %.4f (30 runs)" % (w, h, name, ts[15], ts[0], ts[-1]), flush=True)
    rho = hist.view(n, 8)[:, 5]
    print("rectify r=4 at %dx%d: %.2f %% of pixels rectified" % (w, h, 100.0 * float((rho < 1.0).double().mean())))
    sc.close()


def truth(sc, objs, n, seed):
    kw = dict(dtype=torch.float64, device="cuda")
    sc.set_objects(objs)
    seeds, sums, t = torch.empty(n, **kw), torch.empty(n * 4, **kw), torch.empty(n * 4, **kw)
    api.fill_seeds(seeds.data_ptr(), n, seed)
    sc.render(1024, 0, 1024, seeds.data_ptr(), sums.data_ptr())
    sc.finalize(sums.data_ptr(), t.data_ptr(), 1024)
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(-1, 4)[:, :3]


def ball_shadow():
    W, H, FRAMES, SPP, BALL, STEP, SEED = 64, 48, 8, 8, 7, 0.05, 4100
    objs, tris, grps, cam = scene_inputs("reference", W, H)
    frames = [temporal.move_object(objs, BALL, geom.translate(k * STEP, 0.0, 0.0)) for k in range(FRAMES)]
    sc = api.Scene(0, objs, tris, grps, cam)
    res = {}
    for name, rect in (("rectified", True), ("plain", None)):
        last = None
        rhos = []
        for f in temporal.render_sequence(sc, [cam] * FRAMES, SPP, SEED, temporal=True, objects=frames, rectify=rect):
            torch.cuda.synchronize()
            last = {k: v.cpu().numpy() for k, v in f.items()}
        res[name] = last
    t_last, t_first = truth(sc, frames[-1], W * H, SEED + 1000), truth(sc, frames[0], W * H, SEED + 2000)
    sc.close()
    ids = res["plain"]["feat"].reshape(-1, 12)[:, 7]
    lum = lambda a: a @ np.array([0.2126, 0.7152, 0.0722])
    l1, l0 = lum(t_last), lum(t_first)
    for thr in (0.15, 0.3, 0.5):
        shadow = (ids >= 0) & (ids != BALL) & (np.abs(l1 - l0) > thr * np.maximum(l1, l0))
        rm = lambda a: float(np.sqrt(np.mean((a.reshape(-1, 4)[shadow, :3] - t_last[shadow]) ** 2)))
        print("BALL threshold %.2f: shadow pixels %d (|lum change| between the first and last state, off the ball)" % (thr, shadow.sum()))
        for name in ("rectified", "plain"):
            r = res[name]
            print("BALL %-9s RMSE %.5f  mean N %.3f%s" % (name, rm(r["accumulated"]), r["hist"].reshape(-1, 8)[shadow, 4].mean(),
                  "  mean rho %.4f" % r["rho"][shadow].mean() if "rho" in r else ""))
        print("BALL 8-spp frame RMSE %.5f" % rm(res["plain"]["image"]))
    allhit = ids >= 0
    rm2 = lambda a: float(np.sqrt(np.mean((a.reshape(-1, 4)[allhit, :3] - t_last[allhit]) ** 2)))
    print("BALL all hit pixels: RMSE rectified %.5f plain %.5f frame %.5f" % (rm2(res["rectified"]["accumulated"]),
          rm2(res["plain"]["accumulated"]), rm2(res["plain"]["image"])))


if __name__ == "__main__":
    if "--ball-only" not in sys.argv:
        timings()
    ball_shadow()
