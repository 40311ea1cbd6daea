"""The two frames the motion-reprojection tests share (tests/test_motion_reference.py on the CPU,
tests/test_gpu_reproject_motion.py on the device): the reference scene at 44 x 28 (partial 16 x 16 blocks
and 8 x 8 tiles on both axes), whose larger ball (object 7, radius 0.16, about 5 pixels) stands at x = 0
in frame A and at x = 0.2 in frame B -- a translation parallel to the image plane by more than its radius,
so that without the motion a pixel of the ball finds either another object or a surface point whose
normal is more than 70 degrees off.  The camera is fixed (step 0) or orbited by 3 degrees between the frames.
"""
import numpy as np

from ptmi import geom, temporal
from tests import features_ref
from tests.scene_inputs import scene_inputs

W, H = 44, 28
BALL = 7
SHIFT = (0.2, 0.0, 0.0)
STEPS = (0.0, 3.0)
_cache = {}


def objects():
    """(objects of frame A, objects of frame B)."""
    a = scene_inputs("reference", W, H)[0]
    return a, temporal.move_object(a, BALL, geom.translate(*SHIFT))


def cameras(step):
    cam = scene_inputs("reference", W, H)[3]
    return cam, temporal.orbit_camera(cam, step)


def records(objs, cam):
    """feat[H*W, 12] of the reference scene with these objects through `cam`, by the brute-force comparator."""
    key = (np.ascontiguousarray(objs).tobytes(), np.asarray(cam).tobytes())
    if key not in _cache:
        _, tris, grps, _ = scene_inputs("reference", W, H)
        ref = features_ref.closest_hits(objs, tris, grps, cam, W, H)
        f = np.zeros((W * H, temporal.FEATURE_DOUBLES))
        f[:, 0:3], f[:, 3], f[:, 4:7], f[:, 7], f[:, 8:11] = ref["pos"], ref["t"], ref["normal"], ref["id"], ref["albedo"]
        _cache[key] = f
    return _cache[key]


def interior(feat, cam, cos_min=0.6):
    """Pixels (bool[H*W]) of the ball whose normal is within acos(cos_min) of the direction to the eye: away
    from the silhouette, where a neighbouring pixel may show another object or a steeply turning normal."""
    c = np.asarray(cam).reshape(1)[0]
    eye = np.asarray(c["inverse"], dtype=np.float64).reshape(4, 4)[:3, 3]
    to_eye = eye - feat[:, 0:3]
    to_eye /= np.linalg.norm(to_eye, axis=1, keepdims=True)
    return (feat[:, 7] == BALL) & ((feat[:, 4:7] * to_eye).sum(1) > cos_min)
