"""The device kernel of ptmi_reproject_motion against its numpy statement (ptmi/temporal.py
reproject_reference with `motion`) on two chained real renders of the frames of tests/motion_frames.py:
the reference scene at 44 x 28, 4 spp per frame with different seed streams, the larger ball translated by
0.2 between the frames through Scene.set_objects, the camera fixed and orbited by 3 degrees.  The motion
table is the device's own (ptmi_motion_table), read back and compared with motion_matrices bit for bit.

Tolerance, as tests/test_gpu_reproject.py: every operation is a separately rounded IEEE FP64 one in the
numpy statement's order, so history, out_rgba and out_se are asserted to 1e-9 (of the frame's largest
channel; of max_history for N) outside temporal.undecided, which may mark at most 1 % of the pixels
(tests/test_motion_reference.py checks the cap on the CPU)."""
import numpy as np
import pytest

from ptmi import api, temporal
from tests import motion_frames as mf
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu
W, H = mf.W, mf.H
SPP, CANARY, PAD = 4, -12345.0, 64
_cache = {}


def _frames(step):
    """[(objects, camera, image, se, feat)] of frames A and B, rendered once per camera step."""
    import torch
    if step not in _cache:
        objs_a, objs_b = mf.objects()
        cam_a, cam_b = mf.cameras(step)
        _, tris, grps, _ = scene_inputs("reference", W, H)
        sc = api.Scene(0, objs_a, tris, grps, cam_a)
        out = []
        seq = temporal.render_sequence(sc, [cam_a, cam_b], SPP, 700, temporal=False, objects=[objs_a, objs_b])
        for o, c, f in zip((objs_a, objs_b), (cam_a, cam_b), seq):
            torch.cuda.synchronize()
            out.append((o, c, f["image"].cpu().numpy(), f["se"].cpu().numpy(), f["feat"].cpu().numpy()))
        sc.close()
        _cache[step] = out
    return _cache[step]


def _device(image, se, feat, prev, table, n_obj, params=None, want_rgba=True, want_se=True, plain=False):
    """One ptmi_reproject_motion call (plain: ptmi_reproject): (hist, out_rgba or None, out_se or None), with a
    canary behind every output and around the motion table."""
    import torch
    kw = dict(dtype=torch.float64, device="cuda")
    up = lambda a: torch.tensor(np.ascontiguousarray(a).reshape(-1), **kw)  # noqa: E731
    d_img, d_se, d_feat = up(image), up(se), up(feat)
    prev_hist, prev_feat, prev_cam = up(prev[0]), up(prev[1]), prev[2]
    n = W * H
    bufs = [torch.full((n * k + PAD,), CANARY, **kw) for k in (api.HISTORY_DOUBLES, 4, 1)]
    common = dict(out_rgba_ptr=bufs[1].data_ptr() if want_rgba else 0, out_se_ptr=bufs[2].data_ptr() if want_se else 0,
                  params=params)
    if plain:
        api.reproject(d_img.data_ptr(), d_se.data_ptr(), d_feat.data_ptr(), prev_hist.data_ptr(), prev_feat.data_ptr(),
                      prev_cam, W, H, bufs[0].data_ptr(), **common)
    else:
        d_table = up(table)
        api.reproject_motion(d_img.data_ptr(), d_se.data_ptr(), d_feat.data_ptr(), prev_hist.data_ptr(),
                             prev_feat.data_ptr(), prev_cam, W, H, bufs[0].data_ptr(), d_table.data_ptr(), n_obj, **common)
    torch.cuda.synchronize()
    res = [b.cpu().numpy() for b in bufs]
    for b, k, used in zip(res, (api.HISTORY_DOUBLES, 4, 1), (True, want_rgba, want_se)):
        assert np.all(b[n * k:] == CANARY), "the canary behind an output was overwritten"
        if not used:
            assert np.all(b == CANARY), "an output that was not asked for was written"
    if not plain:
        assert np.array_equal(d_table.cpu().numpy(), np.asarray(table).reshape(-1)), "the motion table was written"
    return res[0][:n * 8], (res[1][:n * 4] if want_rgba else None), (res[2][:n] if want_se else None)


def _first_history(frames):
    o, cam, image, se, feat = frames[0]
    return temporal.reproject_reference(image, se, feat, None, None, None, W, H)[0], feat, cam


def _device_table(prev_objs, cur_objs):
    """ptmi_motion_table into a buffer with canaries on both sides, read back."""
    import torch
    n = len(cur_objs) * api.MOTION_DOUBLES
    buf = torch.full((PAD + n + PAD,), CANARY, dtype=torch.float64, device="cuda")
    api.motion_table(prev_objs, cur_objs, buf.data_ptr() + 8 * PAD)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == CANARY) and np.all(got[PAD + n:] == CANARY)
    return got[PAD:PAD + n].reshape(-1, api.MOTION_DOUBLES)


def test_motion_table_equals_numpy():
    a, b = mf.objects()
    for prev, cur in ((a, b), (b, a), (a, a)):
        assert np.array_equal(_device_table(prev, cur), temporal.motion_matrices(prev, cur))
    c = b.copy()
    c[mf.BALL]["inverse"][14] = 1e-3
    c[0]["transform"][0] = np.nan  # (the linear part: G reads it)
    got, want = _device_table(a, c), temporal.motion_matrices(a, c)
    assert np.array_equal(got, want, equal_nan=True)
    assert got[mf.BALL, 21] == 2.0 and got[0, 21] == 2.0


@pytest.mark.parametrize("step", mf.STEPS)
def test_moved_ball_matches_numpy(step):
    frames = _frames(step)
    prev = _first_history(frames)
    objs_a, objs_b = frames[0][0], frames[1][0]
    _, cam, image, se, feat = frames[1]
    table = _device_table(objs_a, objs_b)
    n_obj = len(objs_b)
    dev = _device(image, se, feat, prev, table, n_obj)
    again = _device(image, se, feat, prev, table, n_obj)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(dev, again)), "two identical calls differ"
    ref = temporal.reproject_reference(image, se, feat, prev[0], prev[1], prev[2], W, H, details=True, motion=table,
                                       n_obj=n_obj)
    keep = ~temporal.undecided(ref[3], W, H).reshape(-1)
    left_out = int((~keep).sum())
    hd, hr = dev[0].reshape(-1, 8), ref[0].reshape(-1, 8)
    fin = np.isfinite(hr[:, :4]).all(1)
    assert np.array_equal(hd[~fin], hr[~fin], equal_nan=True)
    m = keep & fin
    scale = np.abs(hr[fin, :3]).max()
    d_c = np.abs(hd[m, :3] - hr[m, :3]).max() / scale
    d_v = np.abs(hd[m, 3] - hr[m, 3]).max() / scale
    d_n = np.abs(hd[m, 4] - hr[m, 4]).max() / 32.0
    d_rgba = np.abs(dev[1].reshape(-1, 4)[m] - ref[1].reshape(-1, 4)[m]).max() / scale
    d_se = np.abs(dev[2][m] - ref[2][m]).max() / np.sqrt(scale)
    ball = feat.reshape(-1, 12)[:, 7] == mf.BALL
    inside = mf.interior(feat.reshape(-1, 12), cam)
    print("step %g: %d of %d pixels left out; max |device - numpy|: colour %.3e, variance %.3e, N %.3e, out_rgba %.3e, "
          "out_se %.3e; ball pixels %d, interior %d, of them blended %d" %
          (step, left_out, W * H, d_c, d_v, d_n, d_rgba, d_se, ball.sum(), inside.sum(), (hd[inside, 4] == 2.0).sum()))
    assert left_out <= 0.01 * W * H
    assert d_c <= 1e-9 and d_v <= 1e-9 and d_n <= 1e-9 and d_rgba <= 1e-9 and d_se <= 1e-9
    assert np.all(hd[:, 5:] == 0.0)
    assert np.array_equal(dev[1].reshape(-1, 4)[:, :3], hd[:, :3], equal_nan=True) and np.all(dev[1][3::4] == 1.0)
    assert np.array_equal(dev[2], np.sqrt(hd[:, 3]), equal_nan=True)
    # the ball's interior found its history (the records are the device's own; the frames are finite there)
    assert inside.sum() >= 20 and np.all(hd[inside & fin, 4] == 2.0)
    # ... which the parent's function loses
    plain = _device(image, se, feat, prev, None, 0, plain=True)[0].reshape(-1, 8)
    assert np.all(plain[inside & fin, 4] == 1.0)


@pytest.mark.parametrize("step", mf.STEPS)
def test_static_table_equals_ptmi_reproject(step):
    frames = _frames(step)
    prev = _first_history(frames)
    objs_b = frames[1][0]
    _, cam, image, se, feat = frames[1]
    plain = _device(image, se, feat, prev, None, 0, plain=True)
    static = _device(image, se, feat, prev, _device_table(objs_b, objs_b), len(objs_b))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(plain, static))
    short = _device(image, se, feat, prev, _device_table(frames[0][0], objs_b)[:mf.BALL], mf.BALL)  # ids past the table
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(plain, short))


def test_optional_outputs_parameters_and_no_history():
    frames = _frames(0.0)
    prev = _first_history(frames)
    objs_a, objs_b = frames[0][0], frames[1][0]
    _, cam, image, se, feat = frames[1]
    table, n_obj = temporal.motion_matrices(objs_a, objs_b), len(objs_b)
    full = _device(image, se, feat, prev, table, n_obj)
    for want_rgba, want_se in ((False, False), (True, False), (False, True)):
        part = _device(image, se, feat, prev, table, n_obj, want_rgba=want_rgba, want_se=want_se)
        assert np.array_equal(part[0], full[0], equal_nan=True)
        assert part[1] is None or np.array_equal(part[1], full[1], equal_nan=True)
        assert part[2] is None or np.array_equal(part[2], full[2], equal_nan=True)
    params = dict(max_history=1)
    one = _device(image, se, feat, prev, table, n_obj, params)[0].reshape(-1, 8)
    assert np.all(one[np.isfinite(one[:, :4]).all(1), 4] == 1.0)
    # a no-history record, and a singular normal map, reset the ball and nothing else
    ball = feat.reshape(-1, 12)[:, 7] == mf.BALL
    for change in ("state", "G"):
        t2 = table.copy()
        if change == "state":
            t2[mf.BALL, temporal.M_STATE] = temporal.MOTION_NONE
        else:
            t2[mf.BALL, 12:21] = 0.0
        dev = _device(image, se, feat, prev, t2, n_obj)[0].reshape(-1, 8)
        ref = temporal.reproject_reference(image, se, feat, prev[0], prev[1], prev[2], W, H, motion=t2,
                                           n_obj=n_obj)[0].reshape(-1, 8)
        fin = np.isfinite(ref[:, :4]).all(1)
        assert np.all(dev[ball & fin, 4] == 1.0) and np.array_equal(dev[:, 4], ref[:, 4])
        assert np.array_equal(dev[~ball], full[0].reshape(-1, 8)[~ball], equal_nan=True)
