"""Camera sequences on a resident scene and temporal accumulation (ptmi_scene_set_camera,
ptmi_reproject): the temporal half of SVGF, in front of the spatial filter of ptmi/denoise.py.

``reproject_reference`` is the numpy restatement of the device kernel, operation for operation
(csrc/ptmi_kernels.hip reproject_pass): the contract's documentation and the comparator of the GPU
tests.  Every FP64 operation below is an IEEE add, multiply, divide, square root or floor, separately
rounded and in the device's order; the world-to-camera matrix is the same cofactor inverse the library
computes on the host (``cofactor_inverse``).

``orbit_camera`` turns a camera record about the world y axis; ``render_sequence`` renders a list of
cameras from one resident scene and accumulates them.

Limits.  The guides are the pinhole ray through each pixel's centre: depth-of-field blur and sub-pixel
edges are not in them.  The first hit on glass or a mirror reprojects the glass, not what shows through
it, and shading that depends on the view (the reflective and refractive materials) lags by the history
length.  The scene is static: only the camera moves.  The variance needs at least 2 spp per frame (at
1 spp the standard error is +inf and every pixel resets), and it takes the frames for independent
estimates: render them with different seeds.  One GPU.
"""
import math

import numpy as np

from . import geom

FEATURE_DOUBLES = 12  # include/ptmi.h PTMI_FEATURE_DOUBLES
HISTORY_DOUBLES = 8   # PTMI_HISTORY_DOUBLES: colour[3], variance, history length N, 0, 0, 0
H_COL, H_VAR, H_N = slice(0, 3), 3, 4
F_POS, F_T, F_NRM, F_ID = slice(0, 3), 3, slice(4, 7), 7
DEFAULTS = dict(max_history=32, flags=0, normal_cos=0.9, plane_dist=0.02, min_weight=0.05)
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (i, j): the tap (x0 + i, y0 + j), in this order


def params_dict(params=None):
    """The parameters as a dict with the defaults filled in (ptmi_reproject_params): from None, a dict
    of some fields, or an object with those attributes (api.ReprojectParams)."""
    p = dict(DEFAULTS)
    if params is not None:
        for k in p:
            if isinstance(params, dict):
                if k in params:
                    p[k] = params[k]
            elif hasattr(params, k):
                p[k] = getattr(params, k)
    p["max_history"], p["flags"] = int(p["max_history"]), int(p["flags"])
    for k in ("normal_cos", "plane_dist", "min_weight"):
        p[k] = float(p[k])
        if not (np.isfinite(p[k]) and p[k] >= 0.0):
            raise ValueError("bad reproject parameters %r" % (p,))
    if not 1 <= p["max_history"] <= 65536 or p["flags"] != 0:
        raise ValueError("bad reproject parameters %r" % (p,))
    return p


def cofactor_inverse(m):
    """The inverse of a row-major 4 x 4 matrix (16 floats) as the library computes it on the host:
      det3(a) = (a00 (a11 a22 - a12 a21) - a01 (a10 a22 - a12 a20)) + a02 (a10 a21 - a11 a20)
      adj[i][j] = (-1)^(i+j) det3(m without row j and column i)
      det = ((m00 adj00 + m01 adj10) + m02 adj20) + m03 adj30;   inv = adj / det
    Raises ValueError for a singular or non-finite matrix."""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).reshape(16)]

    def det3(r, c):
        a = lambda i, j: m[4 * r[i] + c[j]]  # noqa: E731
        return (a(0, 0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0))) + \
            a(0, 2) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0))

    adj = [0.0] * 16
    for i in range(4):
        for j in range(4):
            r, c = [k for k in range(4) if k != j], [k for k in range(4) if k != i]
            d = det3(r, c)
            adj[4 * i + j] = -d if (i + j) & 1 else d
    det = ((m[0] * adj[0] + m[1] * adj[4]) + m[2] * adj[8]) + m[3] * adj[12]
    if not math.isfinite(det) or det == 0.0:
        raise ValueError("singular or non-finite camera matrix")
    out = np.array([a / det for a in adj], dtype=np.float64)
    if not np.isfinite(out).all():
        raise ValueError("singular or non-finite camera matrix")
    return out


def _finite4(c, v):
    return np.isfinite(c).all(-1) & np.isfinite(v)


def reproject_reference(rgba, se, feat, prev_hist, prev_feat, prev_camera, w, h, params=None, details=False):
    """(hist[W*H*8], out_rgba[W*H*4], out_se[W*H]): the device kernel ptmi_reproject, restated.

    Per pixel p with colour c_p = rgba[p][:3], v_p = se_p * se_p and record (x_p, t_p, n_p, id_p):
      RESET  out = (c_p, v_p, N) with N = 1, or N = 0 when c_p or se_p is not finite, when: prev_hist is
             None; id_p < 0; c_p or se_p not finite; z <= 0; W < min_weight or W == 0 (below).
      T = cofactor_inverse(prev_camera.inverse), rows 0-2:
        q_k = ((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3];   z = -q_2
        fu = (half_width - q_0 / z) / pixel_size - 0.5,  fv = (half_height - q_1 / z) / pixel_size - 0.5
        x0 = floor(fu), wx = fu - x0;  y0 = floor(fv), wy = fv - y0;  bound = plane_dist * t_p
      Taps q = (x0 + i, y0 + j) in the order (0,0), (1,0), (0,1), (1,1); a tap is ACCEPTED when it is
      inside the image, prev_hist[q].N > 0, its colour and variance are finite, prev_feat[q].id == id_p,
        dn = (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= normal_cos   and
        |dd| <= bound,  dd = (n_p.x (x_q.x - x_p.x) + n_p.y (..y)) + n_p.z (..z);   then
        w = (i ? wx : 1 - wx) * (j ? wy : 1 - wy)
        W += w;  r_k += w * (c_q.k - c_p.k);  sv += (w * w) * var_q;  sn += w * N_q
      h_c = c_p + r / W  (the taps' weighted mean, written around c_p so that equal colours stay equal
      bit for bit),  h_var = sv / (W * W),  h_N = sn / W
      N' = min(h_N + 1, max_history),  a = 1 / N',  b = 1 - a
      c' = h_c + a * (c_p - h_c),  var' = (a * a) * v_p + (b * b) * h_var
    out_hist = (c', var', N', 0, 0, 0);  out_rgba = (c', 1.0);  out_se = sqrt(var').

    var' is the variance of the blend when the frames are independent estimates (different seeds).
    details=True also returns a dict of the decisions' test quantities (``undecided``)."""
    p = params_dict(params)
    w, h = int(w), int(h)
    rgba = np.asarray(rgba, dtype=np.float64).reshape(h, w, 4)
    se = np.asarray(se, dtype=np.float64).reshape(h, w)
    feat = np.asarray(feat, dtype=np.float64).reshape(h, w, FEATURE_DOUBLES)
    c, x, t, n, oid = rgba[..., :3], feat[..., F_POS], feat[..., F_T], feat[..., F_NRM], feat[..., F_ID]
    with np.errstate(all="ignore"):
        v = se * se
        fin = np.isfinite(c).all(-1) & np.isfinite(se)
        out_c, out_v, out_n = c.copy(), v.copy(), np.where(fin, 1.0, 0.0)
        info = dict(candidate=np.zeros((h, w), dtype=bool))
        if prev_hist is not None:
            ph = np.asarray(prev_hist, dtype=np.float64).reshape(h * w, HISTORY_DOUBLES)
            pf = np.asarray(prev_feat, dtype=np.float64).reshape(h * w, FEATURE_DOUBLES)
            cam = np.asarray(prev_camera).reshape(1)[0]
            if int(cam["width"]) != w or int(cam["height"]) != h:
                raise ValueError("prev_camera is %dx%d, the frame %dx%d" % (cam["width"], cam["height"], w, h))
            T = cofactor_inverse(cam["inverse"])
            hw, hh, ps = float(cam["half_width"]), float(cam["half_height"]), float(cam["pixel_size"])
            q = [((T[4 * k] * x[..., 0] + T[4 * k + 1] * x[..., 1]) + T[4 * k + 2] * x[..., 2]) + T[4 * k + 3]
                 for k in range(3)]
            z = -q[2]
            cand = fin & ~(oid < 0.0)
            front = cand & (z > 0.0)
            fu = (hw - q[0] / z) / ps - 0.5
            fv = (hh - q[1] / z) / ps - 0.5
            x0, y0 = np.floor(fu), np.floor(fv)
            wx, wy = fu - x0, fv - y0
            bound = p["plane_dist"] * t
            sw, sv, sn, r = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
            taps = []
            for i, j in TAPS:
                tx, ty = x0 + i, y0 + j
                inside = (tx >= 0.0) & (tx < w) & (ty >= 0.0) & (ty < h)
                qi = np.where(inside, ty, 0.0).astype(np.int64) * w + np.where(inside, tx, 0.0).astype(np.int64)
                cq, vq, nq_hist = ph[qi][..., H_COL], ph[qi][..., H_VAR], ph[qi][..., H_N]
                xq, nq, idq = pf[qi][..., F_POS], pf[qi][..., F_NRM], pf[qi][..., F_ID]
                usable = inside & (nq_hist > 0.0) & _finite4(cq, vq) & (idq == oid)
                dn = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                dd = (n[..., 0] * (xq[..., 0] - x[..., 0]) + n[..., 1] * (xq[..., 1] - x[..., 1])) + \
                    n[..., 2] * (xq[..., 2] - x[..., 2])
                ok = front & usable & (dn >= p["normal_cos"]) & (np.abs(dd) <= bound)
                wt = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
                sw = np.where(ok, sw + wt, sw)
                r = np.where(ok[..., None], r + wt[..., None] * (cq - c), r)
                sv = np.where(ok, sv + (wt * wt) * vq, sv)
                sn = np.where(ok, sn + wt * nq_hist, sn)
                taps.append(dict(usable=front & usable, dn=dn, dd=np.abs(dd)))
            blend = front & (sw >= p["min_weight"]) & (sw > 0.0)
            h_c = c + r / sw[..., None]
            h_v, h_n = sv / (sw * sw), sn / sw
            np1 = h_n + 1.0
            n_new = np.where(np1 < float(p["max_history"]), np1, float(p["max_history"]))
            a = 1.0 / n_new
            b = 1.0 - a
            c_new = h_c + a[..., None] * (c - h_c)
            v_new = (a * a) * v + (b * b) * h_v
            out_c = np.where(blend[..., None], c_new, out_c)
            out_v = np.where(blend, v_new, out_v)
            out_n = np.where(blend, n_new, out_n)
            info = dict(candidate=cand, front=front, z=z, t=t, fu=fu, fv=fv, W=sw, bound=bound, taps=taps,
                        blend=blend)
        hist = np.zeros((h, w, HISTORY_DOUBLES))
        hist[..., H_COL], hist[..., H_VAR], hist[..., H_N] = out_c, out_v, out_n
        out_rgba = np.ones((h, w, 4))
        out_rgba[..., :3] = out_c
        out_se = np.sqrt(out_v)
    res = (hist.reshape(-1), out_rgba.reshape(-1), out_se.reshape(-1))
    return res + (info,) if details else res


def undecided(info, w, h, params=None, rtol=1e-9):
    """Pixels (bool[H, W]) one of whose discontinuous decisions hangs on the last bits in the numpy
    statement (``reproject_reference(..., details=True)``): z against 0 (relative to t_p), a usable
    tap's n.n against normal_cos or its plane distance against the bound, and W against min_weight,
    each within `rtol` relative.  (Whether a tap is inside the image is no such decision: it changes
    where fu or fv crosses an integer, and there the tap that comes or goes has weight 0 -- only W
    feels it, and W is tested.)"""
    p = params_dict(params)
    out = np.zeros((h, w), dtype=bool)
    if "z" not in info:
        return out
    with np.errstate(all="ignore"):
        out |= info["candidate"] & (np.abs(info["z"]) <= rtol * np.abs(info["t"]))
        front = info["front"]
        any_usable = np.zeros((h, w), dtype=bool)
        for tap in info["taps"]:
            u = tap["usable"]
            any_usable |= u
            out |= u & (np.abs(tap["dn"] - p["normal_cos"]) <= rtol * p["normal_cos"])
            out |= u & (np.abs(tap["dd"] - info["bound"]) <= rtol * info["bound"])
        out |= front & any_usable & (np.abs(info["W"] - p["min_weight"]) <= rtol * p["min_weight"])
    return out


def orbit_camera(camera_record, degrees):
    """A copy of the camera record whose inverse is rotate_y(degrees) * inverse: the camera orbits about
    the world y axis through the origin (CLCamera carries no from / to to rebuild a view from).  The
    rotation and the product are the scene builder's own (ptmi/geom.py, Go's Sin and Cos), so the CLI's
    --orbit-step gives the same records."""
    cam = np.asarray(camera_record).reshape(1).copy().reshape(())  # (a copy: the caller's record stays)
    rot = geom.rotate_y(float(degrees) * math.pi / 180.0)
    cam["inverse"] = geom.multiply(rot, [float(a) for a in cam["inverse"]])
    return cam


def render_sequence(scene, cameras, samples, seed_stream, temporal=True, denoise=False, reproject_params=None,
                    denoise_params=None, chunks=0, stream=None):
    """Render one frame per camera record of `cameras` from the resident `scene` (api.Scene), per frame k:
    set_camera, fill_seeds(seed_stream + k), render_moments, error_map, finalize, features, and with
    `temporal` reproject against frame k - 1, with `denoise` the a-trous filter on the result.

    A generator: yields per frame a dict of float64 torch tensors on the scene's device -- image, se (the
    frame as rendered), feat, out, out_se (what the frame shows: accumulated and / or filtered; image and
    se themselves without either), and with `temporal` hist (W*H*HISTORY_DOUBLES) and accumulated /
    accumulated_se (the accumulated frame before the filter).  The history and feature ping-pong buffers
    are kept here; a yielded frame's tensors stay valid until the frame after the next is produced, so
    copy what must live longer."""
    import torch
    from . import api

    if samples <= 0:
        raise ValueError("samples must be positive")
    w, h = scene.width, scene.height
    npix = w * h
    st = torch.cuda.current_stream() if stream is None else stream
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        kw = dict(dtype=torch.float64, device="cuda")
        seeds, sums, sq, stats = torch.empty(npix, **kw), torch.empty(npix * 4, **kw), torch.empty(npix, **kw), \
            torch.empty(4, **kw)
        ring = [dict(image=torch.empty(npix * 4, **kw), se=torch.empty(npix, **kw),
                     feat=torch.empty(npix * FEATURE_DOUBLES, **kw), hist=torch.empty(npix * HISTORY_DOUBLES, **kw),
                     accumulated=torch.empty(npix * 4, **kw), accumulated_se=torch.empty(npix, **kw),
                     dn=torch.empty(npix * 4, **kw), dn_se=torch.empty(npix, **kw)) for _ in range(2)]
        work = torch.empty(api.denoise_work_bytes(w, h) // 8, **kw) if denoise else None
    prev, prev_cam = None, None
    for k, cam in enumerate(cameras):
        cur = ring[k & 1]
        scene.set_camera(cam)  # host-blocking: the previous frame's work is done
        with torch.cuda.stream(st):
            api.fill_seeds(seeds.data_ptr(), npix, int(seed_stream) + k, stream=sp)
            scene.render_moments(samples, 0, samples, seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), chunks=chunks,
                                 stream=sp)
            api.error_map(sums.data_ptr(), sq.data_ptr(), w, h, stats.data_ptr(), se_ptr=cur["se"].data_ptr(), stream=sp)
            scene.finalize(sums.data_ptr(), cur["image"].data_ptr(), samples, stream=sp)
            scene.features(cur["feat"].data_ptr(), stream=sp)
            frame = dict(image=cur["image"], se=cur["se"], feat=cur["feat"], out=cur["image"], out_se=cur["se"])
            if temporal:
                api.reproject(cur["image"].data_ptr(), cur["se"].data_ptr(), cur["feat"].data_ptr(),
                              prev["hist"].data_ptr() if prev else 0, prev["feat"].data_ptr() if prev else 0,
                              prev_cam, w, h, cur["hist"].data_ptr(), out_rgba_ptr=cur["accumulated"].data_ptr(),
                              out_se_ptr=cur["accumulated_se"].data_ptr(), params=reproject_params, stream=sp)
                frame.update(hist=cur["hist"], accumulated=cur["accumulated"], accumulated_se=cur["accumulated_se"],
                             out=cur["accumulated"], out_se=cur["accumulated_se"])
            if denoise:
                api.denoise(frame["out"].data_ptr(), frame["out_se"].data_ptr(), cur["feat"].data_ptr(), w, h,
                            cur["dn"].data_ptr(), out_se_ptr=cur["dn_se"].data_ptr(), params=denoise_params, stream=sp,
                            work=work)
                frame.update(out=cur["dn"], out_se=cur["dn_se"])
        prev, prev_cam = cur, np.asarray(cam).reshape(1).copy()
        yield frame
