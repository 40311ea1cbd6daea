"""First-hit feature buffers and the variance-guided a-trous denoiser (ptmi_scene_features,
ptmi_denoise).

``atrous_reference`` is the numpy restatement of the device filter, operation for operation
(csrc/ptmi_image_kernels.hip denoise_start / denoise_pass / denoise_end): the contract's documentation
and the comparator of the GPU tests.  Every FP64 operation below is separately rounded and in the
device's order; ``exp`` is the one operation whose last bits may differ between numpy and the device.

``render_denoised`` renders a frame with moments and denoises it; ``denoise_frame`` denoises a frame
some other loop produced (``error.render_to_noise`` / ``error.render_adaptive`` with ``denoise=True``).

The guides are the pinhole ray through each pixel's centre: depth-of-field blur and sub-pixel edges are
not in them.  With ``guides="first"`` (the default) they are the first hit, which on glass or a mirror
says little about what the pixel shows; ``guides="specular"`` follows the ray through mirrors and glass
to the first surface that is neither (ptmi_scene_features_chain).
"""
import numpy as np

FEATURE_DOUBLES = 12  # include/ptmi.h PTMI_FEATURE_DOUBLES
DEMODULATE = 1        # PTMI_DENOISE_DEMODULATE
F_POS, F_T, F_NRM, F_ID, F_ALB = slice(0, 3), 3, slice(4, 7), 7, slice(8, 11)

DEFAULTS = dict(iterations=5, flags=DEMODULATE, sigma_l=4.0, sigma_d=0.01, normal_power=7)
H_TAPS = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)  # the B3 spline
G_TAPS = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)  # the variance prefilter: 1/4, 1/8, 1/16 as products
ALBEDO_FLOOR = 1e-3
EPS = 1e-12
GUIDES = ("first", "specular")


def trace_guides(scene, feat_ptr, guides="first", stream=0):
    """The guide records of `scene` at feat_ptr: the first hits (ptmi_scene_features) or, with
    guides="specular", the specular chains' final surfaces (ptmi_scene_features_chain, its defaults)."""
    if guides not in GUIDES:
        raise ValueError("guides must be one of %r, got %r" % (GUIDES, guides))
    scene.features(feat_ptr, stream=stream, chain=guides == "specular")


def params_dict(params=None):
    """The filter's parameters as a dict with the defaults filled in (ptmi_denoise_params): from None,
    a dict of some fields, or an object with those attributes (api.DenoiseParams)."""
    p = dict(DEFAULTS)
    if params is None:
        return p
    for k in p:
        if isinstance(params, dict):
            if k in params:
                p[k] = params[k]
        elif hasattr(params, k):
            p[k] = getattr(params, k)
    p["iterations"], p["flags"], p["normal_power"] = int(p["iterations"]), int(p["flags"]), int(p["normal_power"])
    p["sigma_l"], p["sigma_d"] = float(p["sigma_l"]), float(p["sigma_d"])
    if not 1 <= p["iterations"] <= 8 or p["flags"] & ~DEMODULATE or not 0 <= p["normal_power"] <= 16 or \
            not (np.isfinite(p["sigma_l"]) and p["sigma_l"] >= 0.0 and np.isfinite(p["sigma_d"]) and p["sigma_d"] >= 0.0):
        raise ValueError("bad denoise parameters %r" % (p,))
    return p


def lum(c):
    """(0.2126 r + 0.7152 g) + 0.0722 b over the last axis."""
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def _shift(a, ox, oy, fill=0.0):
    """(b, inside): b[y, x] = a[y + oy, x + ox] where that is inside the image, `fill` elsewhere."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), dtype=bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def _floor(a):
    """max(a, 1e-3) as the device writes it: a > 1e-3 ? a : 1e-3 (a NaN gives the floor)."""
    return np.where(a > ALBEDO_FLOOR, a, ALBEDO_FLOOR)


def atrous_pass(c, v, feat, step, p):
    """One a-trous pass at tap distance `step` over the state (c[H, W, 3], v[H, W]); returns the new state.

    For pixel p, with the taps q = p + step * (dx, dy), dx, dy in [-2, 2], dy outermost (row-major):
      vbar = the 3x3 (1/4, 1/8, 1/16) mean of v around p at distance 1 over the taps that are not skipped
             (below), the sum of the products divided by the sum of the weights used;
      sd   = sigma_l * sqrt(vbar < 0 ? 0 : vbar) + 1e-12;    dd_den = sigma_d * t_p + 1e-12
      a tap is SKIPPED when it is outside the image, when its colour or variance is not finite, or when
      exactly one of p, q is a miss (object id < 0); otherwise, hh = h[dx] * h[dy] and
        centre tap:  w = hh
        p a miss:    w = hh * exp(-(|lum(c_p) - lum(c_q)| / sd))
        else:        dn = (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z;  wn = dn > 0 ? dn : 0, squared
                     normal_power times;  dd = (n_p.x (x_q.x - x_p.x) + n_p.y (..y)) + n_p.z (..z)
                     w = ((hh * wn) * exp(-(|dd| / dd_den))) * exp(-(|lum(c_p) - lum(c_q)| / sd))
      sw += w;  sc_k += w * (c_q.k - c_p.k);  s2 += (w * w) * v_q
    c'_p = c_p + sc / sw  (the weighted mean, written around c_p so that equal colours stay equal bit for
    bit),  v'_p = s2 / (sw * sw).  A pixel whose own colour or variance is not finite keeps its state.
    """
    x, t, n, oid = feat[..., F_POS], feat[..., F_T], feat[..., F_NRM], feat[..., F_ID]
    fin = np.isfinite(c).all(-1) & np.isfinite(v)
    miss = oid < 0.0
    with np.errstate(all="ignore"):
        sv, sk = np.zeros_like(v), np.zeros_like(v)
        for gy in range(3):
            for gx in range(3):
                k = G_TAPS[gx] * G_TAPS[gy]
                ox, oy = gx - 1, gy - 1
                cq, inside = _shift(c, ox, oy)
                vq = _shift(v, ox, oy)[0]
                ok = inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & ((_shift(oid, ox, oy)[0] < 0.0) == miss)
                sv = np.where(ok, sv + k * vq, sv)
                sk = np.where(ok, sk + k, sk)
        vbar = sv / sk
        sd = p["sigma_l"] * np.sqrt(np.where(vbar < 0.0, 0.0, vbar)) + EPS
        dd_den = p["sigma_d"] * t + EPS
        lp = lum(c)
        sw, s2, sc = np.zeros_like(v), np.zeros_like(v), np.zeros_like(c)
        for iy in range(5):
            for ix in range(5):
                ox, oy = (ix - 2) * step, (iy - 2) * step
                hh = H_TAPS[ix] * H_TAPS[iy]
                cq, inside = _shift(c, ox, oy)
                vq, xq, nq = _shift(v, ox, oy)[0], _shift(x, ox, oy)[0], _shift(n, ox, oy)[0]
                mq = _shift(oid, ox, oy)[0] < 0.0
                ok = inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & (mq == miss)
                if ox == 0 and oy == 0:
                    w = np.full_like(v, hh)
                else:
                    wl = np.exp(-(np.abs(lp - lum(cq)) / sd))
                    dn = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    wn = np.where(dn > 0.0, dn, 0.0)
                    for _ in range(p["normal_power"]):
                        wn = wn * wn
                    dd = (n[..., 0] * (xq[..., 0] - x[..., 0]) + n[..., 1] * (xq[..., 1] - x[..., 1])) + \
                        n[..., 2] * (xq[..., 2] - x[..., 2])
                    wd = np.exp(-(np.abs(dd) / dd_den))
                    w = np.where(miss, hh * wl, ((hh * wn) * wd) * wl)
                sw = np.where(ok, sw + w, sw)
                s2 = np.where(ok, s2 + (w * w) * vq, s2)
                sc = np.where(ok[..., None], sc + w[..., None] * (cq - c), sc)
        c_new = c + sc / sw[..., None]
        v_new = s2 / (sw * sw)
    return np.where(fin[..., None], c_new, c), np.where(fin, v_new, v)


def atrous_reference(rgba, se, feat, w, h, params=None):
    """(out_rgba[W*H*4], out_se[W*H]): the device filter ptmi_denoise, restated.

    rgba: the frame (ptmi_finalize / ptmi_finalize_counts), se: its standard-error map (ptmi_error_map),
    feat: the first-hit records (ptmi_scene_features, 12 doubles per pixel).

    Start, per pixel:  a_k = albedo_k > 1e-3 ? albedo_k : 1e-3,  m = lum(albedo) > 1e-3 ? lum(albedo) : 1e-3
      with DEMODULATE  c_k = rgb_k / a_k,  v = (se * se) / (m * m);   else  c = rgb,  v = se * se.
    Passes i = 0 .. iterations - 1: atrous_pass at step 2^i.
    End:  with DEMODULATE  rgb'_k = c_k * a_k,  se' = sqrt(v) * m;  else  rgb' = c,  se' = sqrt(v);  alpha 1.0.
    A pixel whose input colour or se is not finite keeps its state through every pass, and the end
    copies its input rgb and se, bit for bit.
    """
    p = params_dict(params)
    w, h = int(w), int(h)
    rgba = np.asarray(rgba, dtype=np.float64).reshape(h, w, 4)
    se = np.asarray(se, dtype=np.float64).reshape(h, w)
    feat = np.asarray(feat, dtype=np.float64).reshape(h, w, FEATURE_DOUBLES)
    rgb, alb = rgba[..., :3], feat[..., F_ALB]
    demod = bool(p["flags"] & DEMODULATE)
    with np.errstate(all="ignore"):
        a, la = _floor(alb), lum(alb)
        m = _floor(la)
        c = rgb / a if demod else rgb.copy()
        v = (se * se) / (m * m) if demod else se * se
        for i in range(p["iterations"]):
            c, v = atrous_pass(c, v, feat, 1 << i, p)
        out = np.ones((h, w, 4))
        out[..., :3] = c * a if demod else c
        out_se = np.sqrt(v) * m if demod else np.sqrt(v)
    keep = ~(np.isfinite(rgb).all(-1) & np.isfinite(se))
    out[..., :3] = np.where(keep[..., None], rgb, out[..., :3])
    out_se = np.where(keep, se, out_se)
    return out.reshape(-1), out_se.reshape(-1)


def normal_image(feat, w, h):
    """RGBA (W*H*4) picture of the feature normals: RGB = n * 0.5 + 0.5 (0.5 on a miss), A = 1."""
    f = np.asarray(feat, dtype=np.float64).reshape(int(h) * int(w), FEATURE_DOUBLES)
    out = np.ones((f.shape[0], 4))
    out[:, :3] = f[:, F_NRM] * 0.5 + 0.5
    return out.reshape(-1)


def denoise_frame(scene, image, se, params=None, stream=None, guides="first"):
    """Denoise a frame of `scene` (api.Scene): `image` (RGBA, W*H*4) and `se` (W*H) are float64 torch
    tensors on the scene's device, as render_to_noise and render_adaptive return them.  Traces the
    feature pass (`guides`: "first" or "specular") and runs the filter; returns (denoised image,
    filtered se, features) as such tensors."""
    import torch
    from . import api

    if guides not in GUIDES:
        raise ValueError("guides must be one of %r, got %r" % (GUIDES, guides))
    npix = scene.width * scene.height
    st = torch.cuda.current_stream() if stream is None else stream
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        kw = dict(dtype=torch.float64, device="cuda")
        feat = torch.empty(npix * FEATURE_DOUBLES, **kw)
        out, out_se = torch.empty(npix * 4, **kw), torch.empty(npix, **kw)
        trace_guides(scene, feat.data_ptr(), guides, stream=sp)
        api.denoise(image.data_ptr(), se.data_ptr(), feat.data_ptr(), scene.width, scene.height, out.data_ptr(),
                    out_se_ptr=out_se.data_ptr(), params=params, stream=sp)
    return out, out_se, feat


def render_denoised(scene, samples, seeds_ptr, params=None, chunks=0, stream=None, guides="first"):
    """Render a `samples`-spp frame of `scene` (api.Scene) with moments and denoise it:
    render_moments -> error_map -> finalize -> features -> denoise, all on one stream.

    Returns (denoised, denoised_se, image, se, feat): float64 torch tensors on the scene's device --
    the filtered RGBA frame and its standard-error map, the frame and map that went in, and the
    guide records (`guides`: "first" or "specular")."""
    import torch
    from . import api

    if samples <= 0:
        raise ValueError("samples must be positive")
    if guides not in GUIDES:
        raise ValueError("guides must be one of %r, got %r" % (GUIDES, guides))
    npix = scene.width * scene.height
    st = torch.cuda.current_stream() if stream is None else stream
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        kw = dict(dtype=torch.float64, device="cuda")
        sums, sq = torch.empty(npix * 4, **kw), torch.empty(npix, **kw)
        se, stats, image = torch.empty(npix, **kw), torch.empty(4, **kw), torch.empty(npix * 4, **kw)
        scene.render_moments(samples, 0, samples, seeds_ptr, sums.data_ptr(), sq.data_ptr(), chunks=chunks, stream=sp)
        api.error_map(sums.data_ptr(), sq.data_ptr(), scene.width, scene.height, stats.data_ptr(),
                      se_ptr=se.data_ptr(), stream=sp)
        scene.finalize(sums.data_ptr(), image.data_ptr(), samples, stream=sp)
        out, out_se, feat = denoise_frame(scene, image, se, params=params, stream=st, guides=guides)
    return out, out_se, image, se, feat
