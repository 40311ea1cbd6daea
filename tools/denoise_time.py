"""DIAGNOSTIC: device time of the feature pass and of the a-trous denoiser, by HIP events.
    python tools/denoise_time.py <scene> [--width W --height H] [--samples N] [--runs R] [--frame-spp S]
Renders an N-spp frame with moments, then times R runs each of ptmi_scene_features and of
ptmi_denoise (default parameters) in both forms of the pass (ptmi_diag_denoise_variant: 0 global
gathers, 1 LDS-staged steps 1 and 2), and each pass count 1..5 of the default form; beside them the
kernel time of one S-spp frame of the same build.  With --quality LO,HI also the RMSE table:
LO-spp frame and its denoised form against the HI-spp frame of the same seeds, over the hit pixels.
"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pathtracer-ocl_amd")]
import torch  # noqa: E402
from ptmi import api, denoise, layout  # noqa: E402
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
    ap.add_argument("--frame-spp", type=int, default=2048)
    ap.add_argument("--quality", default="")
    a = ap.parse_args()
    w, h = a.width, a.height
    npix = w * h
    fmt = lambda ms: " / ".join("%.3f" % m for m in ms)
    lib = api.load_library()
    sc = api.Scene(0, *scene_inputs(a.scene, w, h))
    seeds = torch.tensor(layout.seeds_go_float64(npix, 1234), dtype=torch.float64, device="cuda")
    print("%s %dx%d, library %s" % (a.scene, w, h, api.LIB_PATH))
    den, den_se, image, se, feat = denoise.render_denoised(sc, a.samples, seeds.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    kw = dict(dtype=torch.float64, device="cuda")
    out, out_se = torch.empty(npix * 4, **kw), torch.empty(npix, **kw)
    work = torch.empty(api.denoise_work_bytes(w, h) // 8, **kw)
    print("features            ms: %s" % fmt(event_ms(lambda: sc.features(feat.data_ptr(), stream=st), a.runs)))

    def run(params=None):
        api.denoise(image.data_ptr(), se.data_ptr(), feat.data_ptr(), w, h, out.data_ptr(), out_se_ptr=out_se.data_ptr(),
                    params=params, stream=st, work=work)

    for variant, name in ((0, "global gathers"), (1, "LDS steps 1, 2"), (0, "global gathers"), (1, "LDS steps 1, 2")):
        prev = lib.ptmi_diag_denoise_variant(variant)
        print("denoise, %s ms: %s" % (name, fmt(event_ms(run, a.runs))))
        lib.ptmi_diag_denoise_variant(prev)
    for it in range(1, 6):
        print("denoise, %d passes (default form) ms: %s" % (it, fmt(event_ms(lambda: run(dict(iterations=it)), 3))))
    if a.frame_spp:
        sums = torch.empty(npix * 4, **kw)
        S = a.frame_spp
        sc.render(S, 0, S, seeds.data_ptr(), sums.data_ptr(), stream=st)
        torch.cuda.synchronize()
        sc.set_timing(True)
        ms = []
        for _ in range(3):
            sc.render(S, 0, S, seeds.data_ptr(), sums.data_ptr(), stream=st)
            ms.append(sc.kernel_time()[0])
        sc.set_timing(False)
        print("%d-spp frame kernel ms: %s" % (S, fmt(ms)))
    if a.quality:
        lo_list, hi = a.quality.split(":")
        hi = int(hi)
        sums, ref = torch.empty(npix * 4, **kw), torch.empty(npix * 4, **kw)
        sc.render(hi, 0, hi, seeds.data_ptr(), sums.data_ptr(), stream=st)
        sc.finalize(sums.data_ptr(), ref.data_ptr(), hi, stream=st)
        hit = feat.view(npix, 12)[:, 7] >= 0
        rmse = lambda x: float((x.view(npix, 4)[hit][:, :3] - ref.view(npix, 4)[hit][:, :3]).square().mean().sqrt())
        for lo in [int(x) for x in lo_list.split(",")]:
            d, _, n, _, _ = denoise.render_denoised(sc, lo, seeds.data_ptr())
            print("quality vs %d spp: %4d spp RMSE %.5f, denoised %.5f, ratio %.3f" % (hi, lo, rmse(n), rmse(d),
                                                                                   rmse(d) / rmse(n)))
    sc.close()


if __name__ == "__main__":
    main()
