"""Properties of the numpy statements of ptmi_motion_table and ptmi_reproject_motion (ptmi/temporal.py
motion_matrices, reproject_reference with `motion`) on CPU, on the frames of tests/motion_frames.py: first-hit
records from the brute-force comparator, synthetic colours and standard errors.

Bounds.  States, resets and history lengths are exact by the operation order (with every accepted tap at
N = 1 the two sums W and sum w N are the same additions, so h_N = 1 and N' = 2 exactly).  B and G of a
translation are products of an exactly representable scale with its rounded reciprocal: entries are
asserted to 1e-12 absolute, 1e4 x their rounding."""
import numpy as np
import pytest

from ptmi import geom, temporal
from tests import motion_frames as mf

W, H = mf.W, mf.H


def frame(rng):
    rgba = np.ones((H * W, 4))
    rgba[:, :3] = rng.rand(H * W, 3) * 2.0
    return rgba.reshape(-1), 0.05 + rng.rand(H * W)


def test_identical_records_are_static():
    a, _ = mf.objects()
    m = temporal.motion_matrices(a, a)
    assert m.shape == (len(a), temporal.MOTION_DOUBLES)
    assert np.all(m[:, temporal.M_STATE] == temporal.MOTION_STATIC) and np.all(m[:, 22:] == 0.0)


def test_translation_maps_points_and_keeps_normals():
    a, b = mf.objects()
    m = temporal.motion_matrices(a, b)
    state = m[:, temporal.M_STATE]
    assert state[mf.BALL] == temporal.MOTION_MOVED
    assert np.all(np.delete(state, mf.BALL) == temporal.MOTION_STATIC)
    B, G = m[mf.BALL, :12].reshape(3, 4), m[mf.BALL, 12:21].reshape(3, 3)
    rng = np.random.RandomState(3)
    for _ in range(8):
        p = rng.randn(3)
        p /= np.linalg.norm(p)  # a point of the unit sphere in object space, and its object-space normal
        new = np.asarray(geom.multiply_by_tuple(list(b[mf.BALL]["transform"]), list(p) + [1.0]))[:3]
        old = np.asarray(geom.multiply_by_tuple(list(a[mf.BALL]["transform"]), list(p) + [1.0]))[:3]
        assert np.abs(B @ np.append(new, 1.0) - old).max() <= 1e-12
        assert np.abs(new - old - np.asarray(mf.SHIFT)).max() <= 1e-12
        g = G @ p
        assert np.abs(g / np.linalg.norm(g) - p).max() <= 1e-12
    # and the way back is the inverse motion
    back = temporal.motion_matrices(b, a)[mf.BALL, :12].reshape(3, 4)
    assert np.abs(back[:, 3] + B[:, 3]).max() <= 1e-12


def test_projective_and_non_finite_records_have_no_history():
    a, b = mf.objects()
    c = b.copy()
    c[mf.BALL]["inverse"][14] = 1e-3
    assert temporal.motion_matrices(a, c)[mf.BALL, temporal.M_STATE] == temporal.MOTION_NONE
    c = b.copy()
    c[mf.BALL]["inverse"][3] = np.nan
    assert temporal.motion_matrices(a, c)[mf.BALL, temporal.M_STATE] == temporal.MOTION_NONE
    c = a.copy()
    c[mf.BALL]["transform"][12] = 0.5  # prev.transform's bottom row
    assert temporal.motion_matrices(c, b)[mf.BALL, temporal.M_STATE] == temporal.MOTION_NONE
    with pytest.raises(ValueError):
        temporal.motion_matrices(a, b[:-1])


def _two_frames(step, seed=4):
    a, b = mf.objects()
    cam_a, cam_b = mf.cameras(step)
    rng = np.random.RandomState(seed)
    feat_a, feat_b = mf.records(a, cam_a), mf.records(b, cam_b)
    rgba_a, se_a = frame(rng)
    rgba_b, se_b = frame(rng)
    hist_a = temporal.reproject_reference(rgba_a, se_a, feat_a, None, None, None, W, H)[0]
    return a, b, cam_a, cam_b, feat_a, feat_b, hist_a, rgba_b, se_b


def test_static_table_equals_the_call_without_one():
    a, b, cam_a, cam_b, feat_a, feat_b, hist_a, rgba_b, se_b = _two_frames(3.0)
    plain = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H)
    static = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H,
                                          motion=temporal.motion_matrices(a, a), n_obj=len(a))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(plain, static))
    # ids outside the table are static too
    short = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H,
                                         motion=temporal.motion_matrices(a, b)[:mf.BALL], n_obj=mf.BALL)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(plain, short))


def test_moved_ball_keeps_its_history_only_with_its_motion():
    a, b, cam_a, cam_b, feat_a, feat_b, hist_a, rgba_b, se_b = _two_frames(0.0)
    n_obj = len(a)
    inside = mf.interior(feat_b, cam_b)
    uncovered = (feat_a[:, 7] == mf.BALL) & (feat_b[:, 7] != mf.BALL) & (feat_b[:, 7] >= 0)
    assert inside.sum() >= 20 and uncovered.sum() >= 20, (inside.sum(), uncovered.sum())
    moved = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H,
                                         motion=temporal.motion_matrices(a, b), n_obj=n_obj)[0].reshape(-1, 8)
    static = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H,
                                          motion=temporal.motion_matrices(b, b), n_obj=n_obj)[0].reshape(-1, 8)
    print("ball pixels %d, interior %d, uncovered %d; blended with motion %d, with a static table %d" %
          ((feat_b[:, 7] == mf.BALL).sum(), inside.sum(), uncovered.sum(), (moved[inside, 4] == 2.0).sum(),
           (static[inside, 4] > 1.0).sum()))
    assert np.all(moved[inside, 4] == 2.0)
    assert np.all(static[inside, 4] == 1.0)
    assert np.all(moved[uncovered, 4] == 1.0) and np.all(static[uncovered, 4] == 1.0)
    # what stands still is untouched by the ball's record
    still = feat_b[:, 7] != mf.BALL
    assert np.array_equal(moved[still], static[still])


def test_no_history_record_resets():
    a, b, cam_a, cam_b, feat_a, feat_b, hist_a, rgba_b, se_b = _two_frames(0.0)
    table = temporal.motion_matrices(a, b)
    table[mf.BALL, temporal.M_STATE] = temporal.MOTION_NONE
    out = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H, motion=table,
                                       n_obj=len(a))[0].reshape(-1, 8)
    ball = feat_b[:, 7] == mf.BALL
    assert np.all(out[ball, 4] == 1.0)
    assert np.array_equal(out[ball, :3], rgba_b.reshape(-1, 4)[ball, :3])
    assert (out[~ball, 4] == 2.0).sum() > 0.5 * (~ball).sum()  # the rest of the frame keeps its history
    # a singular normal map (G = 0) resets as well
    table = temporal.motion_matrices(a, b)
    table[mf.BALL, 12:21] = 0.0
    out = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H, motion=table,
                                       n_obj=len(a))[0].reshape(-1, 8)
    assert np.all(out[ball, 4] == 1.0)


@pytest.mark.parametrize("step", mf.STEPS)
def test_few_decisions_hang_on_the_last_bits(step):
    """The frames of tests/test_gpu_reproject_motion.py: the pixels the GPU comparison may leave out
    (temporal.undecided) stay within its cap of 1 % of a frame."""
    a, b, cam_a, cam_b, feat_a, feat_b, hist_a, rgba_b, se_b = _two_frames(step)
    *_, info = temporal.reproject_reference(rgba_b, se_b, feat_b, hist_a, feat_a, cam_a, W, H, details=True,
                                            motion=temporal.motion_matrices(a, b), n_obj=len(a))
    left_out = int(temporal.undecided(info, W, H).sum())
    print("step %g: %d of %d pixels undecided" % (step, left_out, W * H))
    assert left_out <= 0.01 * W * H
