"""DIAGNOSTIC: what per-tile adaptive sampling saves against the whole-frame noise-target loop.
    [PTMI_LIB=...] python tools/adaptive_time.py <scene> [--width W --height H] [--max-samples N]
                       [--batch B] [--at SPP[,SPP...]] [--runs R]
    [PTMI_LIB=...] python tools/adaptive_time.py <scene> --plain [--max-samples N] [--runs R]
    python tools/adaptive_time.py <scene> --once SPP      (one adaptive run, for a kernel trace)
Default mode: renders the frame once with target 0 (render_to_noise), takes the relative noise its
history shows at each --at sample count as a target, and for each target runs render_to_noise and
render_adaptive R times (after one warm-up each): wall time, samples traced, the final
stats[0] / stats[2] and the active tiles per round.
--plain: kernel time (HIP events) of R frames of render and of render_moments, alternated; needs
only entry points the library had before adaptive sampling, so it runs against an older build.
"""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pathtracer-ocl_amd")]
import torch  # noqa: E402
from ptmi import api, error, layout  # noqa: E402
from tests.scene_inputs import scene_inputs  # noqa: E402


def timed(fn, runs):
    fn()  # warm-up
    torch.cuda.synchronize()
    out, ms = None, []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--at", default="256,1024")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    w, h, S, B = a.width, a.height, a.max_samples, a.batch
    npix = w * h
    sc = api.Scene(0, *scene_inputs(a.scene, w, h))
    seeds = torch.tensor(layout.seeds_go_float64(npix, 1234), dtype=torch.float64, device="cuda")
    fmt = lambda ms: " / ".join("%.2f" % m for m in ms)
    print("%s %dx%d, library %s" % (a.scene, w, h, api.LIB_PATH))

    if a.plain:
        sums = torch.empty(npix * 4, dtype=torch.float64, device="cuda")
        sq = torch.empty(npix, dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        plain = lambda: sc.render(S, 0, S, seeds.data_ptr(), sums.data_ptr(), stream=st)
        mom = lambda: sc.render_moments(S, 0, S, seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), stream=st)
        plain(), mom()
        torch.cuda.synchronize()
        sc.set_timing(True)
        res = {"render": [], "render_moments": []}
        for _ in range(a.runs):
            for name, fn in (("render", plain), ("render_moments", mom)):
                fn()
                res[name].append(sc.kernel_time()[0])
        for name in res:
            print("%-15s %d spp kernel ms: %s" % (name, S, fmt(res[name])))
        sc.close()
        return

    _, _, _, hist = error.render_to_noise(sc, S, B, 0.0, seeds.data_ptr())
    if a.once:
        target = hist[a.once // B - 1] * (1 + 1e-9)
        _, _, counts, ah = error.render_adaptive(sc, S, B, target, seeds.data_ptr())
        print("once: target %.6g, %d rounds, %d samples" % (target, len(ah), int(counts.sum().item())))
        sc.close()
        return
    for spp in [int(x) for x in a.at.split(",")]:
        target = hist[spp // B - 1] * (1 + 1e-9)  # the uniform loop stops at this batch
        (_, _, done, uh), ums = timed(lambda: error.render_to_noise(sc, S, B, target, seeds.data_ptr()), a.runs)
        (_, _, counts, ah), ams = timed(lambda: error.render_adaptive(sc, S, B, target, seeds.data_ptr()), a.runs)
        counts = counts.cpu().numpy()
        tiles_max = int((counts.reshape(h, w)[::8, ::8] == S).sum())
        print("target %.6g (the frame's relative noise at %d spp)" % (target, spp))
        print("  render_to_noise: %d spp, %d rounds, %.4g Msamples, final ratio %.6g, wall ms %s"
              % (done, len(uh), done * npix / 1e6, uh[-1], fmt(ums)))
        print("  render_adaptive: max %d spp, mean %.1f spp, %d rounds, %.4g Msamples, final ratio %.6g, "
              "%d tiles at max, wall ms %s" % (counts.max(), counts.mean(), len(ah), counts.sum() / 1e6, ah[-1][2],
                                                 tiles_max, fmt(ams)))
        print("  active tiles per round: %s" % [n for n, _, _ in ah])
    sc.close()


if __name__ == "__main__":
    main()
