"""The caches render_frame keeps between renders of one resident scene -- the diagonal owned-tile list and the
mesh scenes' dispatch order -- and what invalidates them: a sequence of renders on one scene object, each bit
for bit the same call on a freshly created scene.  (tests/test_work_plan.py sees the plans; this sees the
resources built from them.)

The teapot at 32 x 24 (4 x 3 tiles: stride 2 takes the diagonal ownership) and 4 spp, chunks = 2."""
import numpy as np
import pytest

from ptmi import api, layout, temporal
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu

W, H, SPP, CHUNKS = 32, 24, 4, 2
LIST = [2, 5, 11]


def _render(sc, call):
    import torch
    kw = dict(dtype=torch.float64, device="cuda")
    seeds = torch.tensor(layout.seeds_go_float64(W * H, 11), **kw)
    sums, sq = torch.full((W * H * 4,), -1.0, **kw), torch.full((W * H,), -1.0, **kw)
    if call == "list":
        t = torch.tensor(LIST, dtype=torch.int32, device="cuda")
        sc.render_tiles(SPP, 0, SPP, t.data_ptr(), len(LIST), seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(),
                        chunks=CHUNKS)
    else:
        stride, offset = call
        sc.render(SPP, 0, SPP, seeds.data_ptr(), sums.data_ptr(), tile_stride=stride, tile_offset=offset, chunks=CHUNKS)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), sq.cpu().numpy()


def test_a_sequence_of_renders_equals_fresh_scenes():
    objs, tris, grps, cam_a = scene_inputs("teapot", W, H)
    cam_b = temporal.orbit_camera(cam_a, 20.0)

    def fresh(cam, call):
        sc = api.Scene(0, objs, tris, grps, cam)
        out = _render(sc, call)
        sc.close()
        return out

    sc = api.Scene(0, objs, tris, grps, cam_a)
    assert sc.tile_ownership(2) == "diagonal"
    frames = []
    for call in ((2, 0), (2, 1), (1, 0), "list", (2, 0)):
        got, want = _render(sc, call), fresh(cam_a, call)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), call
        frames.append(got[0])
    sc.set_camera(cam_b)
    for call in ((2, 0), (1, 0)):
        got, want = _render(sc, call), fresh(cam_b, call)
        assert np.array_equal(got[0], want[0]), ("after set_camera", call)
    sc.close()
    # the renders are not trivially equal: the two shares differ, and together they are the full frame
    assert not np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[4])
    assert np.array_equal(frames[0] + frames[1], frames[2])
    assert frames[3].reshape(H, W, 4)[..., 3].sum() == len(LIST) * 64 * SPP  # the listed tiles' sample counts
