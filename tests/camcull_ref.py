"""Brute-force comparator of the camera-ray stage's candidate masks (csrc/ptmi_camcull.h), shared by
tests/test_camcull_host.py and tests/test_gpu_camcull.py: numpy doubles, every tile's footprint sampled
on an n x n grid that includes its corners and edges."""
import numpy as np

from ptmi import geom, layout
from tests import test_gpu_stages as st

EPS = 1e-4  # tracer.cl:4
ST_ZEROS = (1, 2, 4, 6, 8, 9, 12, 13, 14)


def object_bits(objs):
    """{list index: mask bit} of the planes (list order) and the scale+translate spheres (list order)."""
    bits, p, q = {}, 0, 0
    for i, o in enumerate(objs):
        if o["type"] == 0:
            bits[i], p = p, p + 1
        elif o["type"] == 1 and all(o["inverse"][k] == 0.0 for k in ST_ZEROS):
            bits[i], q = 16 + q, q + 1
    return bits, p, q


def candidates(objs, cam, n=17):
    """-> {bit: bool[tiles_y, tiles_x]}: some sampled ray of the tile records the object (t > EPSILON)."""
    cam = np.asarray(cam).reshape(1).view(layout.CAMERA_DTYPE)[0]
    w, h = int(cam["width"]), int(cam["height"])
    tx, ty = (w + 7) // 8, (h + 7) // 8
    m = np.asarray(cam["inverse"], dtype=np.float64).reshape(4, 4)
    origin = m[:3, 3]
    u = np.linspace(0.0, 8.0, n)
    xs = (8.0 * np.arange(tx)[:, None] + u[None, :])[None, :, None, :]  # [1, tx, 1, n]
    ys = (8.0 * np.arange(ty)[:, None] + u[None, :])[:, None, :, None]  # [ty, 1, n, 1]
    a = cam["half_width"] - cam["pixel_size"] * xs + 0.0 * ys
    b = cam["half_height"] - cam["pixel_size"] * ys + 0.0 * xs
    v = np.stack([m[r, 0] * a + m[r, 1] * b - m[r, 2] + m[r, 3] - origin[r] for r in range(3)], axis=-1)
    d = v / np.linalg.norm(v, axis=-1, keepdims=True)
    bits, _, _ = object_bits(objs)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, bit in bits.items():
            inv = np.asarray(objs[i]["inverse"], dtype=np.float64).reshape(4, 4)
            if bit < 16:
                oy = inv[1, :3] @ origin + inv[1, 3]
                dy = d @ inv[1, :3]
                cand = (np.abs(dy) > EPS) & (-oy / dy > EPS)
            else:
                o = np.diag(inv)[:3] * origin + inv[:3, 3]
                dd = d * np.diag(inv)[:3]
                qa, qb, qc = (dd * dd).sum(-1), 2.0 * (dd @ o), o @ o - 1.0
                disc = qb * qb - 4.0 * qa * qc
                sq = np.sqrt(np.maximum(disc, 0.0))
                cand = (disc > 0.0) & (((-qb - sq) / (2 * qa) > EPS) | ((-qb + sq) / (2 * qa) > EPS))
            out[bit] = cand.any(axis=(2, 3))
    return out


def check_masks(masks, objs, cam):
    """The hard condition (every cleared bit is candidate-free) and the non-vacuity condition (a bit kept on
    a candidate-free tile has a candidate within one tile).  -> (cleared bits, kept-though-free pairs)."""
    rec = np.asarray(cam).reshape(1).view(layout.CAMERA_DTYPE)[0]
    tx, ty = (int(rec["width"]) + 7) // 8, (int(rec["height"]) + 7) // 8
    masks = np.asarray(masks).reshape(ty, tx)
    _, n_pl, n_sp = object_bits(objs)
    cleared = loose = 0
    for bit, cand in candidates(objs, cam).items():
        kept = ((masks >> np.uint32(bit)) & 1).astype(bool)
        assert not np.any(~kept & cand), "bit %d cleared on tiles %s where a ray records the object" % (
            bit, np.argwhere(~kept & cand).tolist())
        cleared += int((~kept).sum())
        near = np.zeros_like(cand)
        pad = np.pad(cand, 1)
        for dy in range(3):
            for dx in range(3):
                near |= pad[dy:dy + ty, dx:dx + tx]
        free = kept & ~cand
        loose += int(free.sum())
        assert not np.any(free & ~near), "bit %d kept on tiles %s, no candidate within one tile" % (
            bit, np.argwhere(free & ~near).tolist())
    used = sum(1 << b for b in list(range(n_pl)) + [16 + q for q in range(n_sp)])
    assert np.all((masks | np.uint32(used)) == np.uint32(0xFFFFFFFF)), "a bit without an object is cleared"
    return cleared, loose


def plane_counts(masks, objs):
    """Mask statistics: {kept planes: tiles}, {kept st spheres: tiles}."""
    _, n_pl, n_sp = object_bits(objs)
    masks = np.asarray(masks, dtype=np.uint32)
    pl = np.array([bin(int(v) & ((1 << n_pl) - 1)).count("1") for v in masks])
    sp = np.array([bin((int(v) >> 16) & ((1 << n_sp) - 1)).count("1") for v in masks])
    return ({int(k): int((pl == k).sum()) for k in np.unique(pl)}, {int(k): int((sp == k).sum()) for k in np.unique(sp)})


# ---- the cases both tests use -------------------------------------------------------------------
OUTSIDE = ((1.6, 0.9, -2.6), (0, 0, 0))       # outside the box, looking in
ABOVE = ((0.2, 1.2, -0.6), (0, 0.4, 0))       # outside too, above the ceiling: the light's cap pokes through it,
                                              # the one view from outside the infinite walls that is not black
ON_FLOOR = ((0, -0.4, -1.5), (0, 0.05, 0))    # origin on the floor plane: its origin term is an exact zero
OTHER = ((0.3, 0.2, -1.2), (-0.1, -0.1, 0.1))
NEAR_BALL = ((0, -0.24, -0.5), (0, -0.24, -0.30))  # 0.2 from the centre of the 0.16 ball: it fills the view


def reference(w, h, frm=st.STD_FROM, to=st.STD_TO):
    return st._reference(w, h, frm, to)


def many_planes(w, h):
    """The fullest object list the boundary takes (16 objects, tracer.cl:846): the light, a ball and 14
    planes -- the box and nine tilted planes behind its walls.  (A scene with 17 planes, past the mask's 16
    plane bits, cannot be created: the classifier's no-culling branch for it is unreachable through the ABI.)"""
    tilted = [st._plane(geom.translate(0, -.5 - 0.1 * k, 0), geom.rotate_z(0.05 * (k - 4)), geom.rotate_x(0.04 * k))
              for k in range(9)]
    objs = [st._light(), st.FLOOR(), st.CEIL(), st.LEFT(), st.RIGHT(), st.BACK()] + tilted + [st._ball(*st.BALLS[1])]
    return st._records(objs, st._camera(w, h, st.STD_FROM, st.STD_TO))


def host_cases():
    return {
        "reference-160x120": reference(160, 120),
        "reference-outside": reference(160, 120, *OUTSIDE),
        "reference-above": reference(160, 120, *ABOVE),
        "reference-on-floor": reference(160, 120, *ON_FLOOR),
        "reference-100x75": reference(100, 75),
        "planes-5-no-run": st._plane_scene("5-no-run", 100, 75),
        "planes-3-tilted-first": st._plane_scene("3-tilted-first", 64, 48),
        "spheres-4": st._sphere_scene(4, False, 100, 75),
        "spheres-3-rotated": st._sphere_scene(3, True, 64, 48),
    }
