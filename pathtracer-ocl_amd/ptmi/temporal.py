"""Camera sequences on a resident scene and temporal accumulation (ptmi_scene_set_camera,
ptmi_reproject): the temporal half of SVGF, in front of the spatial filter of ptmi/denoise.py.

``reproject_reference`` is the numpy restatement of the device kernel, operation for operation
(csrc/ptmi_image_kernels.hip reproject_pass): the contract's documentation and the comparator of the GPU
tests.  Every FP64 operation below is an IEEE add, multiply, divide, square root or floor, separately
rounded and in the device's order; the world-to-camera matrix is the same cofactor inverse the library
computes on the host (``cofactor_inverse``).

``orbit_camera`` turns a camera record about the world y axis; ``render_sequence`` renders a list of
cameras from one resident scene and accumulates them.

Limits.  The guides are the pinhole ray through each pixel's centre: depth-of-field blur and sub-pixel
edges are not in them.  The first hit on glass or a mirror reprojects the glass, not what shows through
it, and shading that depends on the view (the reflective and refractive materials) lags by the history
length.  Objects may move between frames (Scene.set_objects, ``move_object``): ``motion_matrices`` and
the `motion` argument of ``reproject_reference`` restate ptmi_motion_table and ptmi_reproject_motion, which
carry each first hit back to where that surface point was.  Only what the first-hit records carry is
followed: shadows, reflections and indirect light that move with an object lag by the history length, and
geometry inside a mesh does not deform.  ``gather_reference`` and ``rectify_reference`` restate
ptmi_history_gather and ptmi_rectify (``render_sequence(rectify=...)``), which test the history found
against the frame over a window of same-object pixels and so bound that lag; they see a change of the
window's mean only, test no window of fewer than min_count such pixels, and take the window's pixels for
independent.  The rendered variance needs at least 2 spp per frame (at 1 spp the standard error is +inf and every
pixel resets), and it takes the frames for independent estimates: render them with different seeds.
``variance_reference`` restates ptmi_variance_estimate (``render_sequence(variance="estimated")``), which
estimates each frame's standard error from the moments of each surface point's frames or, where that history is
short, from a window of same-surface pixels: 1 spp is then a normal input.  Both estimates take real changes
(view-dependent shading, moving lights; shading gradients and texture inside the window) for noise and then
overestimate, and the moment history is not rectified.  One GPU.
"""
import math

import numpy as np

from . import geom

FEATURE_DOUBLES = 12  # include/ptmi.h PTMI_FEATURE_DOUBLES
HISTORY_DOUBLES = 8   # PTMI_HISTORY_DOUBLES: colour[3], variance, history length N, 0, 0, 0
MOTION_DOUBLES = 24   # PTMI_MOTION_DOUBLES: B rows 0-2 [12], G [9], state, 0, 0 per object
M_STATE = 21
MOTION_STATIC, MOTION_MOVED, MOTION_NONE = 0.0, 1.0, 2.0
H_COL, H_VAR, H_N = slice(0, 3), 3, 4
F_POS, F_T, F_NRM, F_ID = slice(0, 3), 3, slice(4, 7), 7
DEFAULTS = dict(max_history=32, flags=0, normal_cos=0.9, plane_dist=0.02, min_weight=0.05)
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (i, j): the tap (x0 + i, y0 + j), in this order


def _filled(defaults, params):
    """`defaults` with the fields that `params` gives -- None, a dict of some fields, or an object with those
    attributes -- each as its default's type (int or float)."""
    p = {}
    for k, d in defaults.items():
        if isinstance(params, dict):
            v = params.get(k, d)
        else:
            v = getattr(params, k, d)
        p[k] = type(d)(v)
    return p


def _finite_nonneg(p, *keys):
    return all(np.isfinite(p[k]) and p[k] >= 0.0 for k in keys)


def params_dict(params=None):
    """The parameters as a dict with the defaults filled in (ptmi_reproject_params): from None, a dict
    of some fields, or an object with those attributes (api.ReprojectParams)."""
    p = _filled(DEFAULTS, params)
    if not (_finite_nonneg(p, "normal_cos", "plane_dist", "min_weight") and 1 <= p["max_history"] <= 65536 and
            p["flags"] == 0):
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


def motion_matrices(prev_objects, cur_objects):
    """float64[n_obj, MOTION_DOUBLES]: the table ptmi_motion_table writes for the previous and the current
    object records (the same objects in the same order), restated.  Record k:
      [0:12]   rows 0-2 of B = prev.transform * cur.inverse, geom.multiply's order: each entry
               ((a0 b0 + a1 b1) + a2 b2) + a3 b3 -- a current world point -> where that surface point was
      [12:21]  G = L(prev.inverse_transpose) * L(cur.transform)^T, L the upper-left 3 x 3, row-major, each
               entry (a0 b0 + a1 b1) + a2 b2 -- the same map for normals (cur.transform^T undoes
               cur.inverse_transpose)
      [21]     MOTION_STATIC when the 384 bytes of transform, inverse and inverse_transpose are equal in
               both records; MOTION_NONE when the bottom row of cur.inverse or of prev.transform is not
               (0, 0, 0, 1) as values, or an entry of B or G is not finite; else MOTION_MOVED
      [22:24]  0"""
    prev, cur = np.ascontiguousarray(prev_objects).reshape(-1), np.ascontiguousarray(cur_objects).reshape(-1)
    if len(prev) != len(cur):
        raise ValueError("motion_matrices: %d previous and %d current records" % (len(prev), len(cur)))
    out = np.zeros((len(cur), MOTION_DOUBLES))
    with np.errstate(all="ignore"):
        for k in range(len(cur)):
            pt, pit = [np.asarray(prev[k][f], dtype=np.float64) for f in ("transform", "inverse_transpose")]
            ct, ci = [np.asarray(cur[k][f], dtype=np.float64) for f in ("transform", "inverse")]
            for r in range(3):
                for c in range(4):
                    out[k, 4 * r + c] = ((pt[4 * r] * ci[c] + pt[4 * r + 1] * ci[4 + c]) + pt[4 * r + 2] * ci[8 + c]) + \
                        pt[4 * r + 3] * ci[12 + c]
                for c in range(3):
                    out[k, 12 + 3 * r + c] = (pit[4 * r] * ct[4 * c] + pit[4 * r + 1] * ct[4 * c + 1]) + \
                        pit[4 * r + 2] * ct[4 * c + 2]
            same = all(np.asarray(prev[k][f]).tobytes() == np.asarray(cur[k][f]).tobytes()
                       for f in ("transform", "inverse", "inverse_transpose"))
            affine = all(m[12] == 0.0 and m[13] == 0.0 and m[14] == 0.0 and m[15] == 1.0 for m in (ci, pt))
            out[k, M_STATE] = MOTION_STATIC if same else \
                MOTION_MOVED if affine and np.isfinite(out[k, :21]).all() else MOTION_NONE
    return out


def reproject_reference(rgba, se, feat, prev_hist, prev_feat, prev_camera, w, h, params=None, details=False,
                        motion=None, n_obj=0):
    """(hist[W*H*8], out_rgba[W*H*4], out_se[W*H]): the device kernel ptmi_reproject, restated -- and with
    `motion` (motion_matrices' table, n_obj records) ptmi_reproject_motion.

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

    With `motion`, for a candidate pixel whose id k = int(id_p) is below n_obj (a NaN id is not), by record
    k's state: MOTION_STATIC, or k outside the table -- the steps above, unchanged; MOTION_MOVED --
        x' = B (x_p, 1), each row ((b0 x + b1 y) + b2 z) + b3;   m = G n_p, each row (g0 n.x + g1 n.y) + g2 n.z
        l = (m0 m0 + m1 m1) + m2 m2;  RESET unless l > 0 and finite;  n' = m / sqrt(l)
      and x', n' take the places of x_p, n_p in q_k, dn and dd (bound stays plane_dist * t_p); any other
      state -- RESET.

    var' is the variance of the blend when the frames are independent estimates (different seeds).
    details=True also returns a dict of the decisions' test quantities (``undecided``)."""
    return _reproject(rgba, se, feat, prev_hist, prev_feat, prev_camera, w, h, params, details, motion, n_obj, False)


def gather_reference(rgba, se, feat, prev_hist, prev_feat, prev_camera, w, h, params=None, details=False, motion=None,
                     n_obj=0):
    """gathered[W*H*8]: the device kernel ptmi_history_gather, restated: everything ``reproject_reference``
    does up to the blend (one body, ``_reproject``), and per pixel the history as found -- (h_c, h_var, h_N,
    0, 0, 0), the very values that function blends -- or, where it RESETS, (c_p, v_p, N = 0): N = 0 says
    that no history was found.  `motion`, `n_obj` and details=True (then (gathered, info)) as there."""
    res = _reproject(rgba, se, feat, prev_hist, prev_feat, prev_camera, w, h, params, details, motion, n_obj, True)
    return (res[0], res[3]) if details else res[0]


def _history_taps(cand, x, t, n, oid, ph, pf, cam, w, h, p, motion, n_obj):
    """The lookup that ``_reproject`` and ``variance_reference`` share (the device's history_taps): the
    candidates' points carried back by `motion`, projected with the previous camera `cam`, and the four taps
    tested.  ph[h*w, 8] is the previous frame's per-pixel record -- a history or a moment record: slots
    [0:4] must be finite and [4] > 0 for a tap to be usable -- and pf its first-hit records.  Returns
    (front, taps, info): per tap of TAPS a dict(ok=, wt=, rec= the tap's record [h, w, 8], usable=, dn=, dd=),
    and the decisions' test quantities but W and blend, which are the caller's."""
    if int(cam["width"]) != w or int(cam["height"]) != h:
        raise ValueError("prev_camera is %dx%d, the frame %dx%d" % (cam["width"], cam["height"], w, h))
    T = cofactor_inverse(cam["inverse"])
    hw, hh, ps = float(cam["half_width"]), float(cam["half_height"]), float(cam["pixel_size"])
    history = np.ones((h, w), dtype=bool)
    if motion is not None:  # the point and its normal as the previous frame saw them
        mt = np.asarray(motion, dtype=np.float64).reshape(-1, MOTION_DOUBLES)[:int(n_obj)]
        known = cand & (oid < float(n_obj))
        rec = mt[np.where(known, oid, 0.0).astype(np.int64)]
        moved = known & (rec[..., M_STATE] == MOTION_MOVED)
        history = ~(known & (rec[..., M_STATE] != MOTION_MOVED) & (rec[..., M_STATE] != MOTION_STATIC))
        xm = [((rec[..., 4 * k] * x[..., 0] + rec[..., 4 * k + 1] * x[..., 1]) + rec[..., 4 * k + 2] * x[..., 2]) +
              rec[..., 4 * k + 3] for k in range(3)]
        e = [(rec[..., 12 + 3 * k] * n[..., 0] + rec[..., 13 + 3 * k] * n[..., 1]) + rec[..., 14 + 3 * k] * n[..., 2]
             for k in range(3)]
        ln = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        history &= ~(moved & ~((ln > 0.0) & np.isfinite(ln)))
        root = np.sqrt(ln)
        x = np.where(moved[..., None], np.stack(xm, -1), x)
        n = np.where(moved[..., None], np.stack([e[0] / root, e[1] / root, e[2] / root], -1), n)
    q = [((T[4 * k] * x[..., 0] + T[4 * k + 1] * x[..., 1]) + T[4 * k + 2] * x[..., 2]) + T[4 * k + 3]
         for k in range(3)]
    z = -q[2]
    front = cand & history & (z > 0.0)
    fu = (hw - q[0] / z) / ps - 0.5
    fv = (hh - q[1] / z) / ps - 0.5
    x0, y0 = np.floor(fu), np.floor(fv)
    wx, wy = fu - x0, fv - y0
    bound = p["plane_dist"] * t
    taps = []
    for i, j in TAPS:
        tx, ty = x0 + i, y0 + j
        inside = (tx >= 0.0) & (tx < w) & (ty >= 0.0) & (ty < h)
        qi = np.where(inside, ty, 0.0).astype(np.int64) * w + np.where(inside, tx, 0.0).astype(np.int64)
        rq = ph[qi]
        xq, nq, idq = pf[qi][..., F_POS], pf[qi][..., F_NRM], pf[qi][..., F_ID]
        usable = inside & (rq[..., H_N] > 0.0) & _finite4(rq[..., H_COL], rq[..., H_VAR]) & (idq == oid)
        dn = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
        dd = (n[..., 0] * (xq[..., 0] - x[..., 0]) + n[..., 1] * (xq[..., 1] - x[..., 1])) + \
            n[..., 2] * (xq[..., 2] - x[..., 2])
        ok = front & usable & (dn >= p["normal_cos"]) & (np.abs(dd) <= bound)
        wt = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
        taps.append(dict(ok=ok, wt=wt, rec=rq, usable=front & usable, dn=dn, dd=np.abs(dd)))
    return front, taps, dict(candidate=cand, front=front, z=z, t=t, fu=fu, fv=fv, bound=bound, taps=taps)


def _reproject(rgba, se, feat, prev_hist, prev_feat, prev_camera, w, h, params, details, motion, n_obj, gather):
    """The body of reproject_reference (gather=False) and gather_reference (gather=True)."""
    p = params_dict(params)
    w, h = int(w), int(h)
    rgba = np.asarray(rgba, dtype=np.float64).reshape(h, w, 4)
    se = np.asarray(se, dtype=np.float64).reshape(h, w)
    feat = np.asarray(feat, dtype=np.float64).reshape(h, w, FEATURE_DOUBLES)
    c, x, t, n, oid = rgba[..., :3], feat[..., F_POS], feat[..., F_T], feat[..., F_NRM], feat[..., F_ID]
    with np.errstate(all="ignore"):
        v = se * se
        fin = np.isfinite(c).all(-1) & np.isfinite(se)
        out_c, out_v, out_n = c.copy(), v.copy(), np.zeros((h, w)) if gather else np.where(fin, 1.0, 0.0)
        info = dict(candidate=np.zeros((h, w), dtype=bool))
        if prev_hist is not None:
            ph = np.asarray(prev_hist, dtype=np.float64).reshape(h * w, HISTORY_DOUBLES)
            pf = np.asarray(prev_feat, dtype=np.float64).reshape(h * w, FEATURE_DOUBLES)
            cam = np.asarray(prev_camera).reshape(1)[0]
            cand = fin & ~(oid < 0.0)
            front, taps, info = _history_taps(cand, x, t, n, oid, ph, pf, cam, w, h, p, motion, n_obj)
            sw, sv, sn, r = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
            for tap in taps:
                ok, wt = tap["ok"], tap["wt"]
                cq, vq, nq_hist = tap["rec"][..., H_COL], tap["rec"][..., H_VAR], tap["rec"][..., H_N]
                sw = np.where(ok, sw + wt, sw)
                r = np.where(ok[..., None], r + wt[..., None] * (cq - c), r)
                sv = np.where(ok, sv + (wt * wt) * vq, sv)
                sn = np.where(ok, sn + wt * nq_hist, sn)
            blend = front & (sw >= p["min_weight"]) & (sw > 0.0)
            info.update(W=sw, blend=blend)
            h_c = c + r / sw[..., None]
            h_v, h_n = sv / (sw * sw), sn / sw
            np1 = h_n + 1.0
            n_new = np.where(np1 < float(p["max_history"]), np1, float(p["max_history"]))
            a = 1.0 / n_new
            b = 1.0 - a
            c_new = h_c + a[..., None] * (c - h_c)
            v_new = (a * a) * v + (b * b) * h_v
            if gather:  # the history as found
                c_new, v_new, n_new = h_c, h_v, h_n
            out_c = np.where(blend[..., None], c_new, out_c)
            out_v = np.where(blend, v_new, out_v)
            out_n = np.where(blend, n_new, out_n)
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


RECTIFY_DEFAULTS = dict(radius=3, min_count=9, gamma=3.0, max_history=32, flags=0)
H_RHO = 5  # a rectified history's [5]: rho


def rectify_params_dict(params=None):
    """The parameters as a dict with the defaults filled in (ptmi_rectify_params): from None, True, a dict
    of some fields, or an object with those attributes (api.RectifyParams)."""
    p = _filled(RECTIFY_DEFAULTS, None if params is True else params)
    if not (1 <= p["radius"] <= 4 and 0 <= p["min_count"] < 2 ** 32 and _finite_nonneg(p, "gamma") and
            1 <= p["max_history"] <= 65536 and p["flags"] == 0):
        raise ValueError("bad rectify parameters %r" % (p,))
    return p


def rectify_reference(rgba, se, feat, gathered, w, h, params=None, details=False):
    """(hist[W*H*8], out_rgba[W*H*4], out_se[W*H]): the device kernel ptmi_rectify, restated.

    Per pixel p with c_p = rgba[p][:3], v_p = se_p * se_p, id_p = feat[p][7] and gathered record
    (h, hv, hn) (``gather_reference``):
      RESET   c_p or se_p not finite: (c_p, v_p, N = 0);  hn == 0: (c_p, v_p, N = 1); rho = 1.
      WINDOW  taps q = p + (dx, dy), dy outer, dx inner, both in [-radius, radius]; ACCEPTED when inside the
              image, id_q == id_p (a NaN id matches nothing), c_q and se_q finite, gathered_q.N > 0; in tap
              order   m += 1;  a_k += c_q.k - c_p.k;  b_k += h_q.k - c_p.k;  sv += v_q;  sh += hv_q
      TEST    d_k = (b_k - a_k) / m;  d2 = (d_0 d_0 + d_1 d_1) + d_2 d_2;  V = (sv + sh) / (m m);
              T2 = (gamma gamma) V.  If m >= min_count and d2 > T2:
                rho = sqrt(T2 / d2);  f = 1 - rho;  h'_k = h_k - f d_k;  hn' = rho hn
              else rho = 1, h' = h, hn' = hn (bit for bit; a NaN compares false).  hv stays.
      BLEND   N' = min(hn' + 1, max_history);  a = 1 / N';  b = 1 - a;  c' = h' + a (c_p - h');
              var' = (a a) v_p + (b b) hv       -- reproject_reference's, in its operations and order.
    out_hist = (c', var', N', rho, 0, 0);  out_rgba = (c', 1.0);  out_se = sqrt(var').
    details=True also returns dict(m=, d2=, T2=, rho=) as [H, W] arrays."""
    p = rectify_params_dict(params)
    w, h, r = int(w), int(h), p["radius"]
    rgba = np.asarray(rgba, dtype=np.float64).reshape(h, w, 4)
    se = np.asarray(se, dtype=np.float64).reshape(h, w)
    oid = np.asarray(feat, dtype=np.float64).reshape(h, w, FEATURE_DOUBLES)[..., F_ID]
    g = np.asarray(gathered, dtype=np.float64).reshape(h, w, HISTORY_DOUBLES)
    c, hc, hv, hn = rgba[..., :3], g[..., H_COL], g[..., H_VAR], g[..., H_N]
    with np.errstate(all="ignore"):
        v = se * se
        fin = np.isfinite(c).all(-1) & np.isfinite(se)
        usable = fin & (hn > 0.0)

        def shifted(a, dx, dy, fill):
            """a[y + dy, x + dx], `fill` outside the image."""
            out = np.full(a.shape, fill, dtype=a.dtype)
            ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            out[yd, xd] = a[ys, xs]
            return out

        m = np.zeros((h, w), dtype=np.int64)
        sa, sb, sv, sh = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ok = shifted(usable, dx, dy, False) & (shifted(oid, dx, dy, np.nan) == oid)
                m = np.where(ok, m + 1, m)
                sa = np.where(ok[..., None], sa + (shifted(c, dx, dy, 0.0) - c), sa)
                sb = np.where(ok[..., None], sb + (shifted(hc, dx, dy, 0.0) - c), sb)
                sv = np.where(ok, sv + shifted(v, dx, dy, 0.0), sv)
                sh = np.where(ok, sh + shifted(hv, dx, dy, 0.0), sh)
        md = m.astype(np.float64)
        d = (sb - sa) / md[..., None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        t2 = (p["gamma"] * p["gamma"]) * ((sv + sh) / (md * md))
        blend = fin & (hn != 0.0)
        rect = blend & (m >= p["min_count"]) & (d2 > t2)
        rho = np.where(rect, np.sqrt(t2 / d2), 1.0)
        f = 1.0 - rho
        h_c = np.where(rect[..., None], hc - f[..., None] * d, hc)
        h_n = np.where(rect, rho * hn, hn)
        np1 = h_n + 1.0
        n_new = np.where(np1 < float(p["max_history"]), np1, float(p["max_history"]))
        a = 1.0 / n_new
        b = 1.0 - a
        c_new = h_c + a[..., None] * (c - h_c)
        v_new = (a * a) * v + (b * b) * hv
        hist = np.zeros((h, w, HISTORY_DOUBLES))
        hist[..., H_COL] = np.where(blend[..., None], c_new, c)
        hist[..., H_VAR] = np.where(blend, v_new, v)
        hist[..., H_N] = np.where(blend, n_new, np.where(fin, 1.0, 0.0))
        hist[..., H_RHO] = rho
        out_rgba = np.ones((h, w, 4))
        out_rgba[..., :3] = hist[..., H_COL]
        out_se = np.sqrt(hist[..., H_VAR])
    res = (hist.reshape(-1), out_rgba.reshape(-1), out_se.reshape(-1))
    return res + (dict(m=m, d2=d2, T2=t2, rho=rho),) if details else res


MOMENT_DOUBLES = 8  # PTMI_MOMENT_DOUBLES: mean colour[3], mean of (r^2 + g^2) + b^2, N, source, sigma^2, 0
V_MEAN, V_SQ, V_N, V_SRC, V_VAR = slice(0, 3), 3, 4, 5, 6
SRC_NONE, SRC_TEMPORAL, SRC_SPATIAL, SRC_FALLBACK = 0.0, 1.0, 2.0, 3.0
VARIANCE_DEFAULTS = dict(max_history=32, min_temporal=4, radius=3, min_count=9, flags=0, normal_cos=0.9,
                         plane_dist=0.02, min_weight=0.05, window_normal_cos=0.9)


def variance_params_dict(params=None):
    """The parameters as a dict with the defaults filled in (ptmi_variance_params): from None, a dict of some
    fields, or an object with those attributes (api.VarianceParams)."""
    p = _filled(VARIANCE_DEFAULTS, params)
    if not (_finite_nonneg(p, "normal_cos", "plane_dist", "min_weight", "window_normal_cos") and
            1 <= p["max_history"] <= 65536 and 2 <= p["min_temporal"] <= 65536 and 1 <= p["radius"] <= 4 and
            2 <= p["min_count"] < 2 ** 32 and p["flags"] == 0):
        raise ValueError("bad variance parameters %r" % (p,))
    return p


def variance_reference(rgba, se, feat, prev_mom, prev_feat, prev_camera, w, h, params=None, details=False, motion=None,
                       n_obj=0):
    """(mom[W*H*8], out_se[W*H]): the device kernel ptmi_variance_estimate, restated -- the standard error of
    this frame's pixels estimated from the moments of each surface point's frames, or, where that history is
    too short, from a window of same-surface pixels of this frame.  `se` (the map as rendered) may be None.

    Per pixel p with colour c = rgba[p][:3], s = (c_r c_r + c_g c_g) + c_b c_b and record (x_p, t_p, n_p, id_p):
      NOT FINITE  c not finite: mom = (c, s, N = 0, 0, 0, 0), out_se = se_p (+inf without `se`).
      GATHER  ``reproject_reference``'s lookup on the previous frame's moment records (one body,
              ``_history_taps``: the projection, the taps in its order, its acceptance tests and resets, with
              `motion` its states); over the accepted taps, W += w and
                r_k += w * (mu_q.k - c_k);  r2 += w * (mu2_q - s);  sn += w * N_q
              h_mu = c + r / W,  h_mu2 = s + r2 / W,  h_N = sn / W  (plain weighted means, written around c and s).
      BLEND   reset (no prev_mom, a miss, z <= 0, W < min_weight or W == 0, motion state 2): mu' = c, mu2' = s,
              N' = 1.  Else N' = min(h_N + 1, max_history), a = 1 / N',
              mu' = h_mu + a * (c - h_mu),  mu2' = h_mu2 + a * (s - h_mu2).
      TEMPORAL  N' >= min_temporal:  d = mu2' - ((mu'_r mu'_r + mu'_g mu'_g) + mu'_b mu'_b),
              var = (d < 0 ? 0 : d) * (N' / (N' - 1)),  source 1.
      SPATIAL otherwise, over this frame: taps q = p + (dx, dy), dy outer, dx inner, both in [-radius, radius];
              ACCEPTED when inside the image, c_q finite, id_q == id_p (a NaN id matches nothing; misses match
              misses) and, unless id_p < 0,  (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= window_normal_cos.
              In tap order, with D = c_q - c:  m += 1;  e_k += D_k;  b += (D_r D_r + D_g D_g) + D_b D_b.
              m >= min_count:  E = e / m,  d = b / m - ((E_r E_r + E_g E_g) + E_b E_b),
              var = (d < 0 ? 0 : d) * (m / (m - 1)),  source 2.
      FALLBACK  else, source 3:  var = se_p * se_p when `se` is given and se_p is finite, else var = s.
    mom = (mu', mu2', N', source, var, 0);  out_se = sqrt(var).

    var estimates the variance of THIS frame's pixel value: sqrt(var) is what the consumers of se expect.
    details=True also returns ``_history_taps``' dict with W and blend (``undecided``), walk (bool[H, W]: the
    pixels that took the window) and window_gap (the smallest |n_p.n_q - window_normal_cos| over the taps that
    the normal test alone decides, inf where there is none): ``variance_undecided``."""
    p = variance_params_dict(params)
    w, h, rad = int(w), int(h), p["radius"]
    rgba = np.asarray(rgba, dtype=np.float64).reshape(h, w, 4)
    se = None if se is None else np.asarray(se, dtype=np.float64).reshape(h, w)
    feat = np.asarray(feat, dtype=np.float64).reshape(h, w, FEATURE_DOUBLES)
    c, x, t, n, oid = rgba[..., :3], feat[..., F_POS], feat[..., F_T], feat[..., F_NRM], feat[..., F_ID]
    with np.errstate(all="ignore"):
        s = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
        fin = np.isfinite(c).all(-1)
        mu, mu2, n_new = c.copy(), s.copy(), np.where(fin, 1.0, 0.0)
        info = dict(candidate=np.zeros((h, w), dtype=bool))
        if prev_mom is not None:
            ph = np.asarray(prev_mom, dtype=np.float64).reshape(h * w, MOMENT_DOUBLES)
            pf = np.asarray(prev_feat, dtype=np.float64).reshape(h * w, FEATURE_DOUBLES)
            cam = np.asarray(prev_camera).reshape(1)[0]
            cand = fin & ~(oid < 0.0)
            front, taps, info = _history_taps(cand, x, t, n, oid, ph, pf, cam, w, h, p, motion, n_obj)
            sw, r2, sn, r = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
            for tap in taps:
                ok, wt = tap["ok"], tap["wt"]
                sw = np.where(ok, sw + wt, sw)
                r = np.where(ok[..., None], r + wt[..., None] * (tap["rec"][..., V_MEAN] - c), r)
                r2 = np.where(ok, r2 + wt * (tap["rec"][..., V_SQ] - s), r2)
                sn = np.where(ok, sn + wt * tap["rec"][..., V_N], sn)
            blend = front & (sw >= p["min_weight"]) & (sw > 0.0)
            info.update(W=sw, blend=blend)
            h_mu = c + r / sw[..., None]
            h_mu2, h_n = s + r2 / sw, sn / sw
            np1 = h_n + 1.0
            nb = np.where(np1 < float(p["max_history"]), np1, float(p["max_history"]))
            a = 1.0 / nb
            mu = np.where(blend[..., None], h_mu + a[..., None] * (c - h_mu), mu)
            mu2 = np.where(blend, h_mu2 + a * (s - h_mu2), mu2)
            n_new = np.where(blend, nb, n_new)
        temporal = fin & (n_new >= float(p["min_temporal"]))
        d = mu2 - ((mu[..., 0] * mu[..., 0] + mu[..., 1] * mu[..., 1]) + mu[..., 2] * mu[..., 2])
        var_t = np.where(d < 0.0, 0.0, d) * (n_new / (n_new - 1.0))

        def shifted(a, dx, dy, fill):
            """a[y + dy, x + dx], `fill` outside the image."""
            out = np.full(a.shape, fill, dtype=a.dtype)
            ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            out[yd, xd] = a[ys, xs]
            return out

        hit = ~(oid < 0.0)
        m = np.zeros((h, w), dtype=np.int64)
        e, b, gap = np.zeros((h, w, 3)), np.zeros((h, w)), np.full((h, w), np.inf)
        for dy in range(-rad, rad + 1):
            for dx in range(-rad, rad + 1):
                same = shifted(fin, dx, dy, False) & (shifted(oid, dx, dy, np.nan) == oid)
                nq = shifted(n, dx, dy, 0.0)
                dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                ok = same & (~hit | (dot >= p["window_normal_cos"]))
                dl = shifted(c, dx, dy, 0.0) - c
                m = np.where(ok, m + 1, m)
                e = np.where(ok[..., None], e + dl, e)
                b = np.where(ok, b + ((dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2]), b)
                gap = np.where(same & hit, np.minimum(gap, np.abs(dot - p["window_normal_cos"])), gap)
        md = m.astype(np.float64)
        eb = e / md[..., None]
        ds = b / md - ((eb[..., 0] * eb[..., 0] + eb[..., 1] * eb[..., 1]) + eb[..., 2] * eb[..., 2])
        var_s = np.where(ds < 0.0, 0.0, ds) * (md / (md - 1.0))
        walk = fin & ~temporal
        spatial = walk & (m >= p["min_count"])
        fallback = walk & ~spatial
        var_f = s if se is None else np.where(np.isfinite(se), se * se, s)
        var = np.where(temporal, var_t, np.where(spatial, var_s, np.where(fallback, var_f, 0.0)))
        mom = np.zeros((h, w, MOMENT_DOUBLES))
        mom[..., V_MEAN], mom[..., V_SQ], mom[..., V_N] = mu, mu2, n_new
        mom[..., V_SRC] = np.where(temporal, SRC_TEMPORAL, np.where(spatial, SRC_SPATIAL,
                                                                    np.where(fallback, SRC_FALLBACK, SRC_NONE)))
        mom[..., V_VAR] = var
        out_se = np.where(fin, np.sqrt(var), np.inf if se is None else se)
        info.update(walk=walk, window_gap=gap)
    res = (mom.reshape(-1), out_se.reshape(-1))
    return res + (info,) if details else res


def variance_undecided(info, w, h, params=None, rtol=1e-9):
    """``undecided`` for ``variance_reference(..., details=True)``: its lookup's decisions, and for a pixel that
    took the window a tap's n_p.n_q within `rtol` relative of window_normal_cos."""
    p = variance_params_dict(params)
    out = undecided(info, w, h, p, rtol)
    return out | (info["walk"] & (info["window_gap"] <= rtol * p["window_normal_cos"]))


def orbit_camera(camera_record, degrees):
    """A copy of the camera record whose inverse is rotate_y(degrees) * inverse: the camera orbits about
    the world y axis through the origin (CLCamera carries no from / to to rebuild a view from).  The
    rotation and the product are the scene builder's own (ptmi/geom.py, Go's Sin and Cos), so the CLI's
    --orbit-step gives the same records."""
    cam = np.asarray(camera_record).reshape(1).copy().reshape(())  # (a copy: the caller's record stays)
    rot = geom.rotate_y(float(degrees) * math.pi / 180.0)
    cam["inverse"] = geom.multiply(rot, [float(a) for a in cam["inverse"]])
    return cam


def move_object(objects, index, matrix):
    """A copy of the object records whose record `index` carries transform' = matrix * transform,
    inverse' = geom.inverse(transform') and inverse_transpose' = geom.transpose(inverse'): the scene
    builder's own functions, as a shape's set_transform uses them (the CLI's --move-object gives the same
    records through the host library)."""
    out = np.ascontiguousarray(objects).copy()
    t = geom.multiply([float(a) for a in matrix], [float(a) for a in out[index]["transform"]])
    inv = geom.inverse(t)
    out[index]["transform"] = t
    out[index]["inverse"] = inv
    out[index]["inverse_transpose"] = geom.transpose(inv)
    return out


def render_sequence(scene, cameras, samples, seed_stream, temporal=True, denoise=False, reproject_params=None,
                    denoise_params=None, chunks=0, stream=None, objects=None, rectify=None, guides="first",
                    variance="rendered", variance_params=None):
    """Render one frame per camera record of `cameras` from the resident `scene` (api.Scene), per frame k:
    set_camera, fill_seeds(seed_stream + k), render_moments, error_map, finalize, features, and with
    `temporal` reproject against frame k - 1, with `denoise` the a-trous filter on the result.

    `objects`: None (the scene's objects stand still), or an iterable of one array of object records per
    frame.  Frame k then starts with set_objects(objects[k]) before its set_camera, and with `temporal`
    its history is found through motion_table(objects[k - 1], objects[k]) and reproject_motion, which
    follows each object's motion.

    `rectify`: None -- the calls above; True or a dict of ptmi_rectify_params fields (with `temporal`) --
    history_gather (with the motion table when `objects` is given) and then rectify take the place of the
    reprojection call: the history is tested against the frame before the blend, and frames also carry
    rho (W*H, 1.0 where the history was left as found).  max_history is then rectify's.

    `guides`: "first" -- the first-hit records; "specular" -- the specular chains' final surfaces at their
    virtual positions (ptmi_scene_features_chain), which the reprojection, the rectification and the filter
    then use as they use the first hits.  Not together with `objects` (ValueError): a motion record moves
    real points, and a virtual point behind a mirror moves as the mirrored object does.

    `variance`: "rendered" -- every pass takes the frame's standard error from the frame's own samples (the
    error map; +inf at 1 spp, where nothing accumulates); "estimated" -- after the guides each frame runs
    variance_estimate (with the motion table when `objects` is given; `variance_params`: None, an
    api.VarianceParams or a dict of its fields) on a moment ping-pong of its own, and the reprojection or the
    gather and the rectification, and the filter, take the estimated map wherever they took the rendered one.
    Frames then also carry se_est (W*H) and moments (W*H*MOMENT_DOUBLES); se stays the map as rendered, and
    samples = 1 is a normal input.  Without `temporal` and `denoise`, out_se is then se_est, not se: out_se is
    always the standard error that goes with out.

    A generator: yields per frame a dict of float64 torch tensors on the scene's device -- image, se (the
    frame as rendered), feat, out, out_se (what the frame shows: accumulated and / or filtered; image and
    se themselves without either), and with `temporal` hist (W*H*HISTORY_DOUBLES) and accumulated /
    accumulated_se (the accumulated frame before the filter).  The history and feature ping-pong buffers
    are kept here; a yielded frame's tensors stay valid until the frame after the next is produced, so
    copy what must live longer."""
    from .denoise import GUIDES, trace_guides
    if guides not in GUIDES:
        raise ValueError("guides must be one of %r, got %r" % (GUIDES, guides))
    if guides == "specular" and objects is not None:
        raise ValueError("guides=\"specular\" does not follow moving objects (objects=): the motion table moves "
                         "real points, not the virtual ones behind a mirror")
    import torch
    from . import api

    if samples <= 0:
        raise ValueError("samples must be positive")
    if variance not in ("rendered", "estimated"):
        raise ValueError("variance must be \"rendered\" or \"estimated\", got %r" % (variance,))
    est = variance == "estimated"
    var_params = api.variance_params(variance_params_dict(variance_params)) if est else None
    if rectify is not None and rectify is not False and not temporal:
        raise ValueError("rectify needs temporal")
    rect = None if rectify is None or rectify is False or not temporal else \
        api.RectifyParams(**{k: v for k, v in rectify_params_dict(rectify).items()})
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
        motion = torch.empty(api.MOTION_DOUBLES * 16, **kw) if objects is not None and (temporal or est) else None
        gathered = torch.empty(npix * HISTORY_DOUBLES, **kw) if rect is not None else None
        if rect is not None:
            for buf in ring:
                buf["rho"] = torch.empty(npix, **kw)
        if est:
            for buf in ring:
                buf["moments"], buf["se_est"] = torch.empty(npix * MOMENT_DOUBLES, **kw), torch.empty(npix, **kw)
    prev, prev_cam, prev_objs, n_obj = None, None, None, 0
    frame_objects = iter(objects) if objects is not None else None
    for k, cam in enumerate(cameras):
        cur = ring[k & 1]
        if frame_objects is not None:
            objs = np.ascontiguousarray(next(frame_objects)).copy()
            scene.set_objects(objs)  # host-blocking, as set_camera
        scene.set_camera(cam)  # host-blocking: the previous frame's work is done
        if motion is not None and prev is not None:  # (the device is idle: nothing reads the table)
            n_obj = len(objs)
            api.motion_table(prev_objs, objs, motion.data_ptr(), stream=sp)
        with torch.cuda.stream(st):
            api.fill_seeds(seeds.data_ptr(), npix, int(seed_stream) + k, stream=sp)
            scene.render_moments(samples, 0, samples, seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), chunks=chunks,
                                 stream=sp)
            api.error_map(sums.data_ptr(), sq.data_ptr(), w, h, stats.data_ptr(), se_ptr=cur["se"].data_ptr(), stream=sp)
            scene.finalize(sums.data_ptr(), cur["image"].data_ptr(), samples, stream=sp)
            trace_guides(scene, cur["feat"].data_ptr(), guides, stream=sp)
            frame = dict(image=cur["image"], se=cur["se"], feat=cur["feat"], out=cur["image"], out_se=cur["se"])
            se_ptr = cur["se"].data_ptr()  # the standard error the passes below take
            if est:
                moving = motion is not None and prev is not None
                api.variance_estimate(cur["image"].data_ptr(), cur["se"].data_ptr(), cur["feat"].data_ptr(),
                                      prev["moments"].data_ptr() if prev else 0, prev["feat"].data_ptr() if prev else 0,
                                      prev_cam, w, h, cur["moments"].data_ptr(), cur["se_est"].data_ptr(),
                                      motion_ptr=motion.data_ptr() if moving else 0, n_obj=n_obj if moving else 0,
                                      params=var_params, stream=sp)
                se_ptr = cur["se_est"].data_ptr()
                frame.update(se_est=cur["se_est"], moments=cur["moments"], out_se=cur["se_est"])
            if rect is not None:
                moving = motion is not None and prev is not None
                api.history_gather(cur["image"].data_ptr(), se_ptr, cur["feat"].data_ptr(),
                                   prev["hist"].data_ptr() if prev else 0, prev["feat"].data_ptr() if prev else 0,
                                   prev_cam, w, h, gathered.data_ptr(), motion_ptr=motion.data_ptr() if moving else 0,
                                   n_obj=n_obj if moving else 0, params=reproject_params, stream=sp)
                api.rectify(cur["image"].data_ptr(), se_ptr, cur["feat"].data_ptr(), gathered.data_ptr(),
                            w, h, cur["hist"].data_ptr(), out_rgba_ptr=cur["accumulated"].data_ptr(),
                            out_se_ptr=cur["accumulated_se"].data_ptr(), params=rect, stream=sp)
                cur["rho"].copy_(cur["hist"].view(npix, HISTORY_DOUBLES)[:, H_RHO])
                frame.update(rho=cur["rho"])
            elif temporal and motion is not None and prev is not None:
                api.reproject_motion(cur["image"].data_ptr(), se_ptr, cur["feat"].data_ptr(),
                                     prev["hist"].data_ptr(), prev["feat"].data_ptr(), prev_cam, w, h,
                                     cur["hist"].data_ptr(), motion.data_ptr(), n_obj,
                                     out_rgba_ptr=cur["accumulated"].data_ptr(),
                                     out_se_ptr=cur["accumulated_se"].data_ptr(), params=reproject_params, stream=sp)
            elif temporal:
                api.reproject(cur["image"].data_ptr(), se_ptr, cur["feat"].data_ptr(),
                              prev["hist"].data_ptr() if prev else 0, prev["feat"].data_ptr() if prev else 0,
                              prev_cam, w, h, cur["hist"].data_ptr(), out_rgba_ptr=cur["accumulated"].data_ptr(),
                              out_se_ptr=cur["accumulated_se"].data_ptr(), params=reproject_params, stream=sp)
            if temporal:
                frame.update(hist=cur["hist"], accumulated=cur["accumulated"], accumulated_se=cur["accumulated_se"],
                             out=cur["accumulated"], out_se=cur["accumulated_se"])
            if denoise:
                api.denoise(frame["out"].data_ptr(), frame["out_se"].data_ptr(), cur["feat"].data_ptr(), w, h,
                            cur["dn"].data_ptr(), out_se_ptr=cur["dn_se"].data_ptr(), params=denoise_params, stream=sp,
                            work=work)
                frame.update(out=cur["dn"], out_se=cur["dn_se"])
        prev, prev_cam = cur, np.asarray(cam).reshape(1).copy()
        if frame_objects is not None:
            prev_objs = objs
        yield frame
