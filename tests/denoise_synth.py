"""Synthetic frames, standard-error maps and first-hit records for the denoiser's tests: small
buffers built in numpy, at 19 x 11 (edge blocks only) and 67 x 66 (more than one block in both
directions, not a multiple of the block; the one size at which some pixel has every step-16 tap
inside the image)."""
import numpy as np

from ptmi.denoise import FEATURE_DOUBLES

SIZES = ((19, 11), (67, 66))


def plane_features(w, h, normal=(0.0, 0.0, 1.0), oid=0.0, albedo=(1.0, 1.0, 1.0), t=5.0):
    """Every pixel hits one plane through the origin-facing grid: positions 0.05 apart inside the
    plane (so n . (x_q - x_p) is exactly 0 for an axis normal), constant t, normal, id and albedo."""
    f = np.zeros((h, w, FEATURE_DOUBLES))
    ys, xs = np.mgrid[0:h, 0:w]
    a, b = xs * 0.05, ys * 0.05
    nrm = np.asarray(normal, dtype=np.float64)
    if nrm[2] != 0.0 and nrm[0] == 0.0:
        f[..., 0], f[..., 1], f[..., 2] = a, b, -t
    else:
        f[..., 0], f[..., 1], f[..., 2] = 0.25, b, a - t
    f[..., 3] = t
    f[..., 4:7] = nrm
    f[..., 7] = oid
    f[..., 8:11] = albedo
    return f


def miss_features(w, h):
    f = np.zeros((h, w, FEATURE_DOUBLES))
    f[..., 7] = -1.0
    return f


def frame(rgb, w, h):
    out = np.ones((h, w, 4))
    out[..., :3] = rgb
    return out


def mixed_case(w, h, seed=11):
    """(rgba[h, w, 4], se[h, w], feat[h, w, 12], marks): a noisy frame over a left plane (normal +z), a
    right plane (10 degrees off it, so its taps get partial weights across the seam), a slab of a third
    plane at right angles, and a block of misses; per-pixel random albedo (one pixel black: the floor);
    one NaN pixel and one pixel with se = +inf (marks: their (y, x))."""
    rng = np.random.RandomState(seed)
    feat = plane_features(w, h)
    tilt = np.array([np.sin(np.radians(10.0)), 0.0, np.cos(np.radians(10.0))])
    x0 = (3 * w) // 5
    feat[:, x0:, 4:7] = tilt
    feat[:, x0:, 7] = 1.0
    feat[:, x0:, 2] -= np.arange(w - x0)[None, :] * 0.05 * np.tan(np.radians(10.0))
    feat[:, x0:, 3] = 5.0 + np.arange(w - x0)[None, :] * 0.01
    y0 = (2 * h) // 3
    feat[y0:, : w // 3] = plane_features(w, h, normal=(1.0, 0.0, 0.0), oid=2.0)[y0:, : w // 3]
    feat[: h // 3, w - w // 4:] = miss_features(w, h)[: h // 3, w - w // 4:]
    hit = feat[..., 7] >= 0.0
    alb = 0.2 + 0.8 * rng.rand(h, w, 3)
    feat[..., 8:11] = np.where(hit[..., None], alb, 0.0)
    base = np.where(feat[..., 7:8] == 1.0, (0.2, 0.5, 0.9), (0.8, 0.6, 0.3))
    base = np.where(feat[..., 7:8] == 2.0, (0.1, 0.9, 0.2), base)
    sigma = 0.02 + 0.2 * rng.rand(h, w)
    rgb = np.where(hit[..., None], base * feat[..., 8:11], 0.05) + sigma[..., None] * rng.randn(h, w, 3) * hit[..., None]
    se = np.where(hit, sigma * np.sqrt(3.0), 0.0)
    marks = dict(nan=(h // 2, w // 4), inf=(h // 2 + 1, w // 2), black=(1, 2))
    rgb[marks["nan"]] = (np.nan, 0.3, 0.3)
    se[marks["inf"]] = np.inf
    feat[marks["black"]][8:11] = 0.0
    return frame(rgb, w, h), se, feat, marks
