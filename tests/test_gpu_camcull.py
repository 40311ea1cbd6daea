"""The masked camera-ray stage (ptmi_kernels.hip find_closest_prims' masked form; csrc/ptmi_camcull.h)
against a kernel without it, bit for bit.

The comparator is test_gpu_stages' (its Pair): the same scene forced onto the material instantiation, which
keeps the regeneration loop and tests every object for every ray.  Beside the frames every case checks that
the masks the device holds equal the host classifier's (ptmi_diag_tile_cull / ptmi_diag_tile_cull_host), that
they pass the brute force of tests/camcull_ref.py, and that the object every pixel's centre ray hits first
(ptmi_scene_features) has its bit set in the pixel's tile.

Frames are 64 x 48 and 100 x 75 at 8 to 24 samples.  A scene with 17 planes cannot be created (the object list
holds 16 objects), so the fullest list stands in for it; the one-quotient form of the parallel pairs at later
bounces is not part of the library, so it has no case here.
"""
import numpy as np
import pytest

from ptmi import api, layout
from tests import camcull_ref as ref
from tests import test_gpu_stages as st

pytestmark = pytest.mark.gpu

F_CYLCUBE = 2


def _masks_and_first_hits(scene, records):
    """Device masks == host masks; brute force; every first-hit object's bit is set.  -> masks"""
    import torch
    objs, tris, grps, cam = records
    masks = scene.tile_cull()
    assert np.array_equal(masks, api.tile_cull_host(objs, tris, grps, cam)), "device and host classifier differ"
    ref.check_masks(masks, objs, cam)
    w, h = scene.width, scene.height
    feat = torch.full((w * h * api.FEATURE_DOUBLES,), -7.0, dtype=torch.float64, device="cuda")
    scene.features(feat.data_ptr())
    torch.cuda.synchronize()
    ids = feat.cpu().numpy().reshape(h, w, api.FEATURE_DOUBLES)[:, :, 7].astype(np.int64)
    bits, _, _ = ref.object_bits(objs)
    tiles = masks.reshape((h + 7) // 8, (w + 7) // 8)
    seen = 0
    for y in range(h):
        for x in range(w):
            if ids[y, x] in bits:
                assert (int(tiles[y // 8, x // 8]) >> bits[ids[y, x]]) & 1, "pixel (%d, %d) hits object %d first" % (
                    x, y, ids[y, x])
                seen += 1
    assert seen > 0
    return masks


def _case(records, spp, own=0, rng=None, paths=False, culled=True):
    p = st.Pair(records, own, rng)
    try:
        masks = _masks_and_first_hits(p.new, records)
        assert bool(np.any(masks != 0xFFFFFFFF)) == culled
        a, b = p.both(spp)
        st._check(a, b, spp, "frame")
        if paths:
            for n in range(spp):
                a, b = p.both(spp, n, n + 1)
                st._equal(a, b, "sample %d" % n)
        return masks
    finally:
        p.close()


@pytest.mark.parametrize("frm,to", [(st.STD_FROM, st.STD_TO), ref.OTHER], ids=["own", "other"])
def test_reference_scene(frm, to):
    _case(ref.reference(64, 48, frm, to), 8, paths=True)


def test_horizon_lines_cross_tile_interiors():
    """100 x 75: the floor / ceiling and left / right horizons run through tile interiors (such tiles keep
    both planes of a pair), and the last tile column and row are partial."""
    records = ref.reference(100, 75)
    masks = _case(records, 8)
    planes, _ = ref.plane_counts(masks, records[0])
    assert planes.get(4, 0) > 0 and planes.get(3, 0) > 0, planes


def test_camera_outside_the_box():
    _case(ref.reference(64, 48, *ref.ABOVE), 8)


def test_camera_on_the_floor_plane():
    _case(ref.reference(64, 48, *ref.ON_FLOOR), 8)


def test_camera_close_to_a_sphere_keeps_it_everywhere():
    records = ref.reference(64, 48, *ref.NEAR_BALL)
    masks = _case(records, 8)
    cand = ref.candidates(records[0], records[3])
    full = [bit for bit in cand if bit >= 16 and cand[bit].all()]  # the 0.16 ball, 0.2 from the origin
    assert len(full) == 1 and np.all((masks >> np.uint32(full[0])) & 1), "the ball covers every tile"


def test_rotated_sphere_and_cylinder_cube_scenes():
    """Objects without a bit are tested for every ray as before; only planes and st spheres are culled."""
    _case(st._sphere_scene(3, True, 64, 48), 8)
    _case(st._cylcube_scene(64, 48), 8, own=F_CYLCUBE)


def test_sixteen_object_scene():
    _case(ref.many_planes(64, 48), 8)


def test_statistical_rng():
    _case(ref.reference(64, 48), 8, rng=api.RNG_XOSHIRO)


def test_render_moments_shards_chunks_and_tile_split():
    import torch
    records = ref.reference(100, 75)
    p = st.Pair(records)
    try:
        s_new, q_new = p.moments(p.new, 12, 0, 12)
        s_old, q_old = p.moments(p.old, 12, 0, 12)
        torch.cuda.synchronize()
        st._check(s_new.cpu().numpy(), s_old.cpu().numpy(), 12, "moment sums")
        st._equal(q_new.cpu().numpy(), q_old.cpu().numpy(), "second moments")
        a, b = p.both(24, 5, 24, chunks=3)  # a shard from s0 > 0 whose tiles are chunk items
        st._check(a, b, 19, "shard [5, 24), chunks = 3")
        whole = s_new.cpu().numpy()
        parts = []
        for off in range(3):  # three ranks' tile shares into zeroed frames: together the one-GPU frame
            out = torch.zeros(p.w * p.h * 4, dtype=torch.float64, device="cuda")
            p.new.render(12, 0, 12, p.seeds.data_ptr(), out.data_ptr(), tile_stride=3, tile_offset=off)
            torch.cuda.synchronize()
            parts.append(out.cpu().numpy())
        owners = sum((q.reshape(-1, 4)[:, 3] != 0).astype(int) for q in parts)
        assert np.all(owners == 1), "every pixel has one owner"
        st._equal(parts[0] + parts[1] + parts[2], whole, "tile split")
    finally:
        p.close()


def test_masks_follow_a_camera_update():
    """A resident scene whose camera changes: the masks are the new camera's, and the frame is that of a scene
    created with it."""
    import torch
    objs, tris, grps, cam_a = ref.reference(64, 48)
    cam_b = ref.reference(64, 48, *ref.ABOVE)[3]
    sc = api.Scene(0, objs, tris, grps, cam_a)
    fresh = api.Scene(0, objs, tris, grps, cam_b)
    try:
        before = sc.tile_cull()
        sc.set_camera(cam_b)
        after = sc.tile_cull()
        assert not np.array_equal(before, after)
        assert np.array_equal(after, fresh.tile_cull())
        assert np.array_equal(after, api.tile_cull_host(objs, tris, grps, cam_b))
        seeds = torch.tensor(layout.seeds_go_float64(64 * 48, 5), dtype=torch.float64, device="cuda")
        frames = []
        for s in (sc, fresh):
            out = torch.empty(64 * 48 * 4, dtype=torch.float64, device="cuda")
            s.render(8, 0, 8, seeds.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            frames.append(out.cpu().numpy())
        assert np.any(frames[0].reshape(-1, 4)[:, :3] != 0.0)
        st._equal(frames[0], frames[1], "updated scene vs fresh scene")
        sc.set_camera(cam_a)
        assert np.array_equal(sc.tile_cull(), before)
    finally:
        sc.close()
        fresh.close()


def test_two_live_scenes_keep_their_own_masks():
    p1 = st.Pair(ref.reference(64, 48))
    p2 = st.Pair(ref.reference(64, 48, *ref.OTHER))
    try:
        m1, m2 = p1.new.tile_cull(), p2.new.tile_cull()
        assert not np.array_equal(m1, m2)
        for _ in range(2):
            a1, b1 = p1.both(8)
            a2, b2 = p2.both(8)
            st._check(a1, b1, 8, "scene 1")
            st._check(a2, b2, 8, "scene 2")
        assert np.array_equal(p1.new.tile_cull(), m1) and np.array_equal(p2.new.tile_cull(), m2)
    finally:
        p1.close()
        p2.close()
