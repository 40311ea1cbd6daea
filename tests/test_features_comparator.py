"""The brute-force feature comparator (tests/features_ref.py) alone, on the CPU: on the frames the GPU
tests use, the pixels it cannot decide itself -- its two nearest candidates within 1e-9 relative in
t -- stay inside the 1 % the GPU comparison may leave out, and it sees hits and (where the scene has
them) misses."""
import numpy as np
import pytest

from tests import features_ref
from tests.scene_inputs import scene_inputs

FRAMES = (("reference", 36, 20), ("teapot", 28, 20), ("envmap", 36, 20))


@pytest.mark.parametrize("scene,w,h", FRAMES)
def test_comparator_decides_its_frames(scene, w, h):
    objs, tris, grps, cam = scene_inputs(scene, w, h)
    ref = features_ref.closest_hits(objs, tris, grps, cam, w, h)
    keep = features_ref.decided(ref)
    assert (~keep).sum() <= 0.01 * w * h
    hit = ref["id"] >= 0
    assert hit.sum() > 0.5 * w * h and len(set(ref["id"][hit])) >= 2
    assert np.abs(np.linalg.norm(ref["normal"][hit], axis=1) - 1.0).max() < 1e-12
    if scene == "teapot":
        assert (np.asarray(objs["type"])[ref["id"][hit]] == 4).any()  # some pixels see the mesh
