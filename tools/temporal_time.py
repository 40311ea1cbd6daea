"""DIAGNOSTIC: device time of the temporal accumulation and host time of a camera update.
    python tools/temporal_time.py <scene> [--width W --height H] [--samples N] [--runs R] [--step DEGREES]
Renders two N-spp frames of an orbit with moments (ptmi/temporal.py render_sequence), then times R runs
of ptmi_reproject on them by HIP events (with history, with both optional outputs), beside ptmi_denoise
on the same frame, and prints the fraction of pixels the timed with-history call blended; then the
wall-clock time of R ptmi_scene_set_camera calls against R ptmi_scene_create calls of the same records
(the device idle before each; the scene's destroy is outside the timed span).
"""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pathtracer-ocl_amd")]
import torch  # noqa: E402
from ptmi import api, temporal  # noqa: E402
from tests.scene_inputs import scene_inputs  # noqa: E402


def event_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step", type=float, default=2.5)
    a = ap.parse_args()
    w, h = a.width, a.height
    npix = w * h
    fmt = lambda ms: " / ".join("%.3f" % m for m in ms)  # noqa: E731
    objs, tris, grps, cam = scene_inputs(a.scene, w, h)
    cams = [temporal.orbit_camera(cam, k * a.step) for k in range(2)]
    print("%s %dx%d, %d triangles, library %s" % (a.scene, w, h, len(tris), api.LIB_PATH))
    sc = api.Scene(0, objs, tris, grps, cam)
    frames = []
    for f in temporal.render_sequence(sc, cams, a.samples, 1234, temporal=True):
        frames.append({k: v.clone() for k, v in f.items()})
    torch.cuda.synchronize()
    prev, cur = frames
    st = torch.cuda.current_stream().cuda_stream
    kw = dict(dtype=torch.float64, device="cuda")
    hist, out, out_se = torch.empty(npix * 8, **kw), torch.empty(npix * 4, **kw), torch.empty(npix, **kw)
    work = torch.empty(api.denoise_work_bytes(w, h) // 8, **kw)

    def reproject(first=False):
        api.reproject(cur["image"].data_ptr(), cur["se"].data_ptr(), cur["feat"].data_ptr(),
                      0 if first else prev["hist"].data_ptr(), 0 if first else prev["feat"].data_ptr(),
                      None if first else cams[0], w, h, hist.data_ptr(), out_rgba_ptr=out.data_ptr(),
                      out_se_ptr=out_se.data_ptr(), stream=st)

    def filt():
        api.denoise(cur["image"].data_ptr(), cur["se"].data_ptr(), cur["feat"].data_ptr(), w, h, out.data_ptr(),
                    out_se_ptr=out_se.data_ptr(), stream=st, work=work)

    for _ in range(2):
        print("reproject, with history ms: %s" % fmt(event_ms(reproject, a.runs)))
        print("reproject, first frame  ms: %s" % fmt(event_ms(lambda: reproject(True), a.runs)))
        print("denoise (default)       ms: %s" % fmt(event_ms(filt, a.runs)))
    reproject()
    torch.cuda.synchronize()
    n = hist.view(npix, 8)[:, 4]
    print("pixels with history after a %.3g-degree step: %.1f %%" % (a.step, 100.0 * float((n > 1.0).double().mean())))
    ms = []
    for k in range(a.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.set_camera(cams[k & 1])
        ms.append((time.perf_counter() - t0) * 1e3)
    print("set_camera              ms: %s" % fmt(ms[1:]))
    sc.close()
    ms = []
    for k in range(a.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s2 = api.Scene(0, objs, tris, grps, cams[k & 1])
        t1 = time.perf_counter()
        s2.close()
        ms.append((t1 - t0) * 1e3)
    print("scene create            ms: %s" % fmt(ms[1:]))


if __name__ == "__main__":
    main()
