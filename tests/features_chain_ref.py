"""A numpy statement of the specular-chain feature pass (ptmi_scene_features_chain, include/ptmi.h) for
scenes of planes and spheres.

Brute force, as tests/features_ref.py: per segment the closest hit over all objects, with the second
nearest candidate kept so that a test can leave out the pixels where the comparator's own choice hangs
on the last bits.  features_ref.closest_hits is written for one ray origin; from the second segment on
every pixel has its own, so the two intersectors are restated here for per-ray origins.

chain_rays follows given rays, chain the camera's pinhole rays.  The rules, per ray, with inside = false,
L = 0, tint m = (1, 1, 1), U = I and k = 0; at each hit (t, pos, eye-facing unit normal n, colour c):
L += t, then the first of
  1. final if the object is emissive (emission[0] > 0) or k == max_chain;
  2. reflectivity >= reflect_min: rd = rd - 2 (rd . n) n from pos, m *= c, U = U (I - 2 n n^T), k++;
  3. refractive index -1 (thin glass): straight on from pos, k++;
  4. refractive index != 1: s2 = nr^2 (1 - (n . eye)^2) with nr = ri inside and 1 / ri outside; s2 > 1 takes
     rule 2's step, otherwise rd = n (nr ci - sqrt(1 - s2)) - eye nr from pos, inside flips, k++;
  5. final otherwise.
A segment starts at pos itself: no hit is taken at t <= EPS, which keeps the surface just left out.
The final record is the hit unfolded along the first ray: position origin + rd0 * L, distance L, normal
U n (negated where it does not face -rd0), the object's index, albedo m * c and k.  A miss on any segment
gives id -1 and zeros, with k kept.
"""
import numpy as np

EPS = 1e-4      # tracer.cl EPSILON
T_MAX = 1024.0  # the closest-hit search starts at 1024
FINAL, REFLECT, THIN, REFRACT, TIR, MISS = range(6)  # what a segment's hit did (the `steps` records)


def _supported(objs):
    for ob in objs:
        if int(ob["type"]) not in (0, 1) or int(ob["is_textured"]) or int(ob["is_textured_nm"]):
            raise ValueError("features_chain_ref handles untextured planes and spheres only")


def closest(objs, ro, rd):
    """Per ray (ro[n, 3], rd[n, 3]): id (-1 miss), t, t2 (second nearest candidate, inf if none)."""
    n = len(ro)
    t1, t2, oid = np.full(n, np.inf), np.full(n, np.inf), np.full(n, -1, dtype=np.int64)

    def push(t, k):
        nonlocal t1, t2, oid
        t = np.where(np.isfinite(t) & (t > EPS) & (t < T_MAX), t, np.inf)
        first = t < t1
        t2 = np.where(first, t1, np.minimum(t2, t))
        t1 = np.where(first, t, t1)
        oid = np.where(first, k, oid)

    with np.errstate(all="ignore"):
        for k, ob in enumerate(objs):
            inv = np.asarray(ob["inverse"], dtype=np.float64).reshape(4, 4)
            o = ro @ inv[:3, :3].T + inv[:3, 3]
            d = rd @ inv[:3, :3].T
            if int(ob["type"]) == 0:
                push(np.where(np.abs(d[:, 1]) > EPS, -o[:, 1] / d[:, 1], np.nan), k)
            else:
                a, b, c = (d * d).sum(1), 2.0 * (d * o).sum(1), (o * o).sum(1) - 1.0
                sq = np.sqrt(b * b - 4.0 * a * c)
                push((-b - sq) / (2.0 * a), k)
                push((-b + sq) / (2.0 * a), k)
    return oid, np.where(oid >= 0, t1, 0.0), t2


def surface(objs, oid, pos, rd):
    """(normal[n, 3], colour[n, 3]) of the hits: the unit world normal facing -rd, and the object's colour."""
    nrm, col = np.zeros_like(pos), np.zeros_like(pos)
    for k, ob in enumerate(objs):
        m = oid == k
        if not m.any():
            continue
        inv = np.asarray(ob["inverse"], dtype=np.float64).reshape(4, 4)
        invt = np.asarray(ob["inverse_transpose"], dtype=np.float64).reshape(4, 4)
        lp = pos[m] @ inv[:3, :3].T + inv[:3, 3]
        on = np.tile([0.0, 1.0, 0.0], (len(lp), 1)) if int(ob["type"]) == 0 else lp
        wn = on @ invt[:3, :3].T
        wn = wn / np.linalg.norm(wn, axis=1, keepdims=True)
        nrm[m] = np.where(((wn * -rd[m]).sum(1) < 0.0)[:, None], -wn, wn)
        col[m] = np.asarray(ob["color"], dtype=np.float64)[:3]
    return nrm, col


def chain_rays(objs, ro, rd, max_chain=8, reflect_min=0.5, rtol=1e-9):
    """Follow the rays (ro[n, 3], rd[n, 3] unit).  Returns id, k, L, pos, normal, albedo as above; `close`:
    rays on which some segment's two nearest candidates were within rtol relative in t, or a refraction's
    s2 within rtol of 1 (the comparator's own choice is then not certain); and `steps`: per segment a dict of
    idx (the rays still going), id, t, normal, rule, s2 (NaN where rule 4 was not reached) and rd_out."""
    _supported(objs)
    ro, rd = np.array(ro, dtype=np.float64), np.array(rd, dtype=np.float64)
    n = len(ro)
    ro0, rd0 = ro.copy(), rd.copy()
    refl = np.array([float(ob["reflectivity"]) for ob in objs])
    ri = np.array([float(ob["refractive_index"]) for ob in objs])
    emis = np.array([float(ob["emission"][0]) for ob in objs])
    L, m, U = np.zeros(n), np.ones((n, 3)), np.tile(np.eye(3), (n, 1, 1))
    k, inside, close = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    out = dict(id=np.full(n, -1, dtype=np.int64), L=np.zeros(n), pos=np.zeros((n, 3)), normal=np.zeros((n, 3)),
               albedo=np.zeros((n, 3)))
    steps, idx = [], np.arange(n)
    while idx.size:
        o, d = ro[idx], rd[idx]
        oid, t, t2 = closest(objs, o, d)
        hit = oid >= 0
        close[idx] |= hit & np.isfinite(t2) & ~(np.abs(t2 - t) > rtol * np.abs(t))
        pos = o + d * t[:, None]
        nv, c = surface(objs, oid, pos, d)
        L[idx] += t
        j = np.where(hit, oid, 0)
        can = hit & ~(emis[j] > 0.0) & (k[idx] < max_chain)
        eye = -d
        nr = np.where(inside[idx], ri[j], 1.0 / ri[j])
        ci = (eye * nv).sum(1)
        s2 = (nr * nr) * (1.0 - ci * ci)
        mirror = can & (refl[j] >= reflect_min)
        thin = can & ~mirror & (ri[j] == -1.0)
        glass = can & ~mirror & ~thin & (ri[j] != 1.0)
        close[idx] |= glass & (np.abs(s2 - 1.0) <= rtol)
        tir = glass & (s2 > 1.0)
        refr = glass & ~tir
        bounce = mirror | tir
        rule = np.full(idx.size, FINAL)
        rule[~hit], rule[mirror], rule[thin], rule[refr], rule[tir] = MISS, REFLECT, THIN, REFRACT, TIR
        with np.errstate(all="ignore"):
            ct = np.sqrt(1.0 - s2)
        d_new = np.where(bounce[:, None], d - 2.0 * (d * nv).sum(1)[:, None] * nv,
                         np.where(refr[:, None], nv * (nr * ci - ct)[:, None] - eye * nr[:, None], d))
        steps.append(dict(idx=idx.copy(), id=oid, t=t, normal=nv, rule=rule, s2=np.where(glass, s2, np.nan),
                          rd_out=d_new))
        # the rays that end here
        fin = hit & ~(bounce | thin | refr)
        f = idx[fin]
        un = np.einsum("nij,nj->ni", U[f], nv[fin])
        un = np.where(((un * rd0[f]).sum(1) > 0.0)[:, None], -un, un)
        out["id"][f], out["L"][f] = oid[fin], L[f]
        out["pos"][f], out["normal"][f], out["albedo"][f] = ro0[f] + rd0[f] * L[f][:, None], un, m[f] * c[fin]
        # the rays that go on
        b = idx[bounce]
        m[b] *= c[bounce]
        nb = nv[bounce]
        U[b] = U[b] - 2.0 * np.einsum("ni,nj->nij", np.einsum("nij,nj->ni", U[b], nb), nb)
        go = bounce | thin | refr
        g = idx[go]
        rd[g] = d_new[go]
        ro[g] = pos[go]
        inside[idx[refr]] = ~inside[idx[refr]]
        k[g] += 1
        idx = g
    out["k"], out["close"], out["steps"] = k, close, steps
    return out


def chain(objs, cam, w, h, max_chain=8, reflect_min=0.5, rtol=1e-9):
    """chain_rays on the pinhole rays through the pixel centres (features_ref.camera_rays); adds origin, dirs."""
    from tests import features_ref
    org, dirs = features_ref.camera_rays(cam, w, h)
    out = chain_rays(objs, np.tile(org, (w * h, 1)), dirs, max_chain, reflect_min, rtol)
    out["origin"], out["dirs"] = org, dirs
    return out


BACK_WALL = 5  # the reference scene's back wall: the plane z = 0.4


def planar_mirror_pair(w, h):
    """(mirror, twin, camera, to_mirror_id): the reference scene with its back wall a perfect mirror
    (shapes.new_mirror: colour 1, reflectivity 1), and its hand-reflected twin -- the wall removed and every
    other object's transform pre-multiplied by the wall's reflection z -> 0.8 - z, so that what the mirror
    shows stands behind where the wall was.  to_mirror_id maps the twin's object ids to the mirror scene's."""
    from ptmi import temporal
    from tests.scene_inputs import scene_inputs
    objs, _, _, cam = scene_inputs("reference", w, h)
    mirror = objs.copy()
    mirror[BACK_WALL]["reflectivity"] = 1.0
    mirror[BACK_WALL]["color"][:3] = 1.0
    flip = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.8, 0.0, 0.0, 0.0, 1.0]
    twin = objs.copy()
    for k in range(len(twin)):
        twin = temporal.move_object(twin, k, flip)
    twin = np.delete(twin, BACK_WALL)
    return mirror, twin, cam, lambda i: np.where(i >= BACK_WALL, i + 1, i)
