"""A brute-force numpy comparator for the first-hit feature pass (ptmi_scene_features).

Independent of the library's traversal: per pixel the closest hit over ALL objects and, for mesh
objects, over ALL of their triangles (no BVH, no box gates), with ray-plane, ray-sphere,
ray-cylinder (open, as the kernel traces them) and ray-cube in object space from the records'
inverses, and Moller-Trumbore for triangles.  It also keeps the second nearest candidate, so a test
can leave out the pixels where the comparator's own choice hangs on the last bits (silhouettes, ties).
"""
import numpy as np

EPS = 1e-4      # tracer.cl EPSILON
T_MAX = 1024.0  # the closest-hit search starts at 1024


def camera_rays(cam, w, h):
    """(origin[3], dirs[h*w, 3]): the pinhole rays through the pixel centres (rayForPixel)."""
    c = np.asarray(cam).reshape(1)[0]
    inv = np.asarray(c["inverse"], dtype=np.float64).reshape(4, 4)
    ys, xs = np.mgrid[0:h, 0:w]
    a = c["half_width"] - c["pixel_size"] * (xs.reshape(-1) + 0.5)
    b = c["half_height"] - c["pixel_size"] * (ys.reshape(-1) + 0.5)
    pix = np.stack([a, b, -np.ones_like(a), np.ones_like(a)], axis=1) @ inv.T
    org = inv @ np.array([0.0, 0.0, 0.0, 1.0])
    d = pix[:, :3] - org[:3]
    return org[:3], d / np.linalg.norm(d, axis=1, keepdims=True)


def _group_triangles(obj, grps):
    """Indices of every triangle under a type-4 object's roots."""
    out, todo = [], [int(g) for g in obj["children"][:int(obj["child_count"])]]
    while todo:
        g = grps[todo.pop()]
        out.extend(range(int(g["tri_offset"]), int(g["tri_offset"]) + int(g["tri_count"])))
        todo.extend(int(k) for k in g["children"] if k > 0)
    return np.array(sorted(out), dtype=np.int64)


def _push(best, t, obj, extra=None):
    """Fold candidates t[n] (NaN / out of range = none) of object `obj` into the two nearest."""
    ok = np.isfinite(t) & (t > EPS) & (t < T_MAX)
    t = np.where(ok, t, np.inf)
    first = t < best["t"]
    best["t2"] = np.where(first, best["t"], np.minimum(best["t2"], t))
    best["t"] = np.where(first, t, best["t"])
    best["id"] = np.where(first, obj, best["id"])
    if extra is not None:
        for k, v in extra.items():
            best[k] = np.where(first.reshape((-1,) + (1,) * (v.ndim - 1)), v, best[k])


def closest_hits(objs, tris, grps, cam, w, h, textures=None, tex_sample=None, uv_maps=None):
    """Per pixel (h*w): id (-1 miss), t, t2 (second nearest candidate, inf if none), pos[3], normal[3],
    albedo[3], textured (bool).  textures: [plane, sphere, cube] image lists; tex_sample(images, s, t,
    layer) -> rgb and uv_maps = (spherical_map, cube_uv) come from the CPU oracle when a scene has
    textured objects."""
    org, dirs = camera_rays(cam, w, h)
    n = w * h
    best = dict(t=np.full(n, np.inf), t2=np.full(n, np.inf), id=np.full(n, -1, dtype=np.int64),
                tri=np.full(n, -1, dtype=np.int64), u=np.zeros(n), v=np.zeros(n))
    o4 = np.append(org, 1.0)
    with np.errstate(all="ignore"):
        for k, ob in enumerate(objs):
            ty = int(ob["type"])
            if ty not in (0, 1, 2, 3, 4):
                continue
            inv = np.asarray(ob["inverse"], dtype=np.float64).reshape(4, 4)
            o = (inv @ o4)[:3]
            d = dirs @ inv[:3, :3].T
            if ty == 0:
                _push(best, np.where(np.abs(d[:, 1]) > EPS, -o[1] / d[:, 1], np.nan), k)
            elif ty == 1:
                a, b, c = (d * d).sum(1), 2.0 * (d @ o), o @ o - 1.0
                sq = np.sqrt(b * b - 4.0 * a * c)
                _push(best, (-b - sq) / (2.0 * a), k)
                _push(best, (-b + sq) / (2.0 * a), k)
            elif ty == 2:
                a = d[:, 0] ** 2 + d[:, 2] ** 2
                b = 2.0 * (o[0] * d[:, 0] + o[2] * d[:, 2])
                sq = np.sqrt(b * b - 4.0 * a * (o[0] ** 2 + o[2] ** 2 - 1.0))
                for t in ((-b - sq) / (2.0 * a), (-b + sq) / (2.0 * a)):
                    y = o[1] + t * d[:, 1]
                    _push(best, np.where((np.abs(a) >= EPS) & (y > ob["min_y"]) & (y < ob["max_y"]), t, np.nan), k)
            elif ty == 3:
                big = np.abs(d) >= EPS
                lo = np.where(big, (-1.0 - o) / d, (-1.0 - o) * np.inf)
                hi = np.where(big, (1.0 - o) / d, (1.0 - o) * np.inf)
                tmin, tmax = np.minimum(lo, hi).max(1), np.maximum(lo, hi).min(1)
                hit = ~(tmin > tmax)
                _push(best, np.where(hit, tmin, np.nan), k)
                _push(best, np.where(hit, tmax, np.nan), k)
            else:
                idx = _group_triangles(ob, grps)
                if idx.size == 0:
                    continue
                T = tris[idx]
                p1, e1, e2 = T["p1"][:, :3], T["e1"][:, :3], T["e2"][:, :3]
                pc = np.cross(d[:, None, :], e2[None, :, :])          # [n, m, 3]
                det = (e1[None] * pc).sum(-1)
                f = 1.0 / det
                s = o[None, :] - p1                                    # [m, 3]
                u = f * (s[None] * pc).sum(-1)
                qc = np.cross(s, e1)                                   # [m, 3]
                v = f * (d @ qc.T)
                t = f * (e2 * qc).sum(-1)[None, :]
                ok = (np.abs(det) >= EPS) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > EPS) & (t < T_MAX)
                t = np.where(ok, t, np.inf)
                j = t.argmin(1)
                r = np.arange(n)
                t1 = t[r, j]
                t[r, j] = np.inf
                _push(best, np.where(np.isfinite(t1), t1, np.nan), k,
                      extra=dict(tri=idx[j], u=u[r, j], v=v[r, j]))
                _push(best, np.where(np.isfinite(t.min(1)), t.min(1), np.nan), k)
    hit = best["id"] >= 0
    t = np.where(hit, best["t"], 0.0)
    pos = np.where(hit[:, None], org[None, :] + dirs * t[:, None], 0.0)
    nrm, alb, textured = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=bool)
    for k, ob in enumerate(objs):
        m = best["id"] == k
        if not m.any():
            continue
        ty = int(ob["type"])
        inv = np.asarray(ob["inverse"], dtype=np.float64).reshape(4, 4)
        invt = np.asarray(ob["inverse_transpose"], dtype=np.float64).reshape(4, 4)
        lp = pos[m] @ inv[:3, :3].T + inv[:3, 3]
        col = np.tile(np.asarray(ob["color"], dtype=np.float64)[:3], (int(m.sum()), 1))
        if ty == 0:
            on = np.tile([0.0, 1.0, 0.0], (lp.shape[0], 1))
        elif ty == 1:
            on = lp
        elif ty == 2:
            dist = lp[:, 0] ** 2 + lp[:, 2] ** 2
            on = np.stack([lp[:, 0], np.zeros(len(lp)), lp[:, 2]], axis=1)
            on[(dist < 1) & (lp[:, 1] >= ob["max_y"] - EPS)] = (0.0, 1.0, 0.0)
            on[(dist < 1) & (lp[:, 1] < ob["max_y"] - EPS) & (lp[:, 1] <= ob["min_y"] + EPS)] = (0.0, -1.0, 0.0)
        elif ty == 3:
            ax = np.abs(lp).argmax(1)
            on = np.zeros_like(lp)
            on[np.arange(len(lp)), ax] = lp[np.arange(len(lp)), ax]
        else:
            T = tris[best["tri"][m]]
            u, v = best["u"][m][:, None], best["v"][m][:, None]
            on = T["n2"][:, :3] * u + T["n3"][:, :3] * v + T["n1"][:, :3] * (1.0 - u - v)
            col = T["color"][:, :3].astype(np.float64)
        if ty in (0, 1, 3) and int(ob["is_textured"]) and tex_sample is not None:
            textured[m] = True
            imgs = (textures or [None] * 3)[{0: 0, 1: 1, 3: 2}[ty]] or []
            for r in range(len(lp)):
                if ty == 0:
                    s, tt = lp[r, 0] * ob["texture_scale_x"], lp[r, 2] * ob["texture_scale_y"]
                elif ty == 1:
                    uu, vv = uv_maps[0](*lp[r])
                    s, tt = uu, 1.0 - vv
                else:
                    s, tt = uv_maps[1](*lp[r])
                col[r] = tex_sample(imgs, float(np.float32(s)), float(np.float32(tt)), float(ob["texture_index"])) \
                    if len(imgs) else (0.0, 0.0, 0.0)
        wn = on @ invt[:3, :3].T
        wn = wn / np.linalg.norm(wn, axis=1, keepdims=True)
        flip = (wn * -dirs[m]).sum(1) < 0.0
        nrm[m] = np.where(flip[:, None], -wn, wn)
        alb[m] = col
    return dict(id=best["id"], t=t, t2=best["t2"], pos=pos, normal=nrm, albedo=alb, textured=textured,
                origin=org, dirs=dirs)


def decided(ref, rtol=1e-9):
    """Pixels whose two nearest candidates are further apart than rtol relative in t (or that miss)."""
    gap = np.abs(ref["t2"] - ref["t"]) > rtol * np.abs(ref["t"])
    return (ref["id"] < 0) | gap | ~np.isfinite(ref["t2"])
