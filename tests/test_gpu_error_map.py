"""The device error map (ptmi_error_map), ptmi_accumulate and the noise-target loop
(ptmi/error.py render_to_noise) against the numpy statement of the formula.

Tolerances: se^2 is sq/n - |mean|^2 scaled by 1/(n - 1); the subtraction cancels, so a rounding
of either term (<= 2^-52 of sq/n) shows in full: |se^2 - reference| <= 1e-12 * sq/n per pixel (the
1/(n - 1) factor is <= 1).  The summaries add non-negative terms: rtol 1e-12.  Infinite and zero
entries are exact."""
import numpy as np
import pytest

from ptmi import api, error, layout
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu


def _device_map(sums, sq, w, h):
    import torch
    ds = torch.tensor(np.asarray(sums, dtype=np.float64).reshape(-1), device="cuda")
    dq = torch.tensor(np.asarray(sq, dtype=np.float64).reshape(-1), device="cuda")
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    se = torch.full((w * h,), -1.0, dtype=torch.float64, device="cuda")
    te = torch.full((tiles,), -1.0, dtype=torch.float64, device="cuda")
    st = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    api.error_map(ds.data_ptr(), dq.data_ptr(), w, h, st.data_ptr(), se_ptr=se.data_ptr(), tile_err_ptr=te.data_ptr())
    torch.cuda.synchronize()
    return se.cpu().numpy(), te.cpu().numpy(), st.cpu().numpy()


def _compare(sums, sq, w, h):
    se, te, st = _device_map(sums, sq, w, h)
    se_b, te_b, st_b = _device_map(sums, sq, w, h)
    for a, b in ((se, se_b), (te, te_b), (st, st_b)):
        assert np.array_equal(a, b, equal_nan=True), "two runs differ"
    r_se, r_te, r_st = error.error_map_reference(sums, sq, w, h)
    n = np.asarray(sums).reshape(-1, 4)[:, 3]
    special = ~np.isfinite(r_se) | (r_se == 0)
    assert np.array_equal(se[special], r_se[special], equal_nan=True)
    fin = ~special
    bound = 1e-12 * np.asarray(sq).reshape(-1)[fin] / n[fin]
    diff = np.abs(se[fin] ** 2 - r_se[fin] ** 2)
    print("se^2: max |diff| / bound %.3e; stats %s reference %s" % ((diff / bound).max() if fin.any() else 0, st, r_st))
    assert np.all(diff <= bound)
    np.testing.assert_allclose(te, r_te, rtol=1e-12, atol=0)
    np.testing.assert_allclose(st, r_st, rtol=1e-12, atol=0)
    assert np.array_equal(te == 0, r_te == 0)
    # without the optional outputs the summaries are the same
    import torch
    ds, dq = torch.tensor(np.asarray(sums).reshape(-1), device="cuda"), torch.tensor(np.asarray(sq), device="cuda")
    st2 = torch.empty(4, dtype=torch.float64, device="cuda")
    api.error_map(ds.data_ptr(), dq.data_ptr(), w, h, st2.data_ptr())
    assert np.array_equal(st2.cpu().numpy(), st)
    return se, te, st


def _rendered(scene, w, h, S, seed):
    import torch
    sc = api.Scene(0, *scene_inputs(scene, w, h))
    seeds = torch.tensor(layout.seeds_go_float64(w * h, seed), dtype=torch.float64, device="cuda")
    sums = torch.empty(w * h * 4, dtype=torch.float64, device="cuda")
    sq = torch.empty(w * h, dtype=torch.float64, device="cuda")
    sc.render_moments(S, 0, S, seeds.data_ptr(), sums.data_ptr(), sq.data_ptr())
    torch.cuda.synchronize()
    sc.close()
    return sums.cpu().numpy(), sq.cpu().numpy()


def test_error_map_on_rendered_frames():
    for scene, w, h, S in (("reference", 36, 20, 13), ("teapot", 28, 20, 24)):
        sums, sq = _rendered(scene, w, h, S, 5)
        se, te, st = _compare(sums, sq, w, h)
        assert st[3] == w * h and st[0] > 0 and st[1] >= st[0] and st[2] > 0
        assert te.shape == (((w + 7) // 8) * ((h + 7) // 8),)


def test_error_map_on_synthetic_buffer():
    """19 x 11 pixels (edge tiles, 6 tiles): not owned, single-sample, constant (zero variance, d a
    rounding away from 0 on either side), and ordinary pixels; one tile wholly not owned."""
    w, h = 19, 11
    rng = np.random.RandomState(7)
    n = rng.randint(2, 40, size=(h, w)).astype(np.float64)
    mean = rng.rand(h, w, 3)
    spread = rng.rand(h, w) * 0.3
    n[:8, :8] = 0          # tile 0: not owned
    n[9, 3] = 0
    n[2, 12] = 1           # +inf
    n[10, 18] = 1
    spread[3:6, 9:15] = 0  # constant pixels: sq / n == |mean|^2 up to rounding
    sums = np.concatenate([mean * n[..., None], n[..., None]], axis=2)
    m2 = ((sums[..., 0] / np.maximum(n, 1)) ** 2 + (sums[..., 1] / np.maximum(n, 1)) ** 2 +
          (sums[..., 2] / np.maximum(n, 1)) ** 2)
    sq = n * (m2 + spread)
    sq[4, 9:15] *= 1 - 2.0 ** -51  # d slightly negative from cancellation
    sq[n == 0] = 0
    se, te, st = _compare(sums.reshape(-1), sq.reshape(-1), w, h)
    se = se.reshape(h, w)
    assert np.all(se[:8, :8] == 0) and te[0] == 0
    assert se[2, 12] == np.inf and se[10, 18] == np.inf
    assert np.all(se[4, 9:15] == 0)
    assert st[3] == np.count_nonzero(n >= 2) and np.isfinite(st).all()


def test_accumulate_equals_numpy():
    import torch
    rng = np.random.RandomState(1)
    a, b = rng.randn(1000 * 4 + 3) * 1e3, rng.randn(1000 * 4 + 3)
    da, db = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    api.accumulate(da.data_ptr(), db.data_ptr(), a.size)
    api.accumulate(da.data_ptr(), db.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(da.cpu().numpy(), a + b)
    assert np.array_equal(db.cpu().numpy(), b)


def test_noise_falls_as_one_over_root_samples():
    """Reference scene 40 x 24: the rms standard error at 256 spp is half that at 64 spp (1/sqrt 4),
    within [0.4, 0.6] for the estimate's own noise (the CPU oracle's frames of three seed sets give 0.502-0.508)."""
    w, h = 40, 24
    st = {}
    for S in (64, 256):
        sums, sq = _rendered("reference", w, h, S, 31)
        st[S] = _device_map(sums, sq, w, h)[2]
    ratio = st[256][0] / st[64][0]
    print("rms se: 64 spp %.6g, 256 spp %.6g, ratio %.4f" % (st[64][0], st[256][0], ratio))
    assert 0.4 <= ratio <= 0.6


def test_render_to_noise():
    import torch
    w, h, S, B = 40, 24, 256, 32
    sc = api.Scene(0, *scene_inputs("reference", w, h))
    seeds = torch.tensor(layout.seeds_go_float64(w * h, 31), dtype=torch.float64, device="cuda")

    def plain(samples_done):
        sums = torch.empty(w * h * 4, dtype=torch.float64, device="cuda")
        out = torch.empty_like(sums)
        sc.render(S, 0, samples_done, seeds.data_ptr(), sums.data_ptr())
        sc.finalize(sums.data_ptr(), out.data_ptr(), samples_done)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    # target 0: every sample
    img, se, done, hist = error.render_to_noise(sc, S, B, 0.0, seeds.data_ptr())
    assert done == S and len(hist) == S // B
    assert all(a > b for a, b in zip(hist, hist[1:])), hist  # ~1/sqrt(n): 8 batches, each well below the last
    full = plain(S)
    img = img.cpu().numpy()
    np.testing.assert_allclose(img, full, rtol=1e-12, atol=0)  # batch boundaries regroup the sums
    assert np.all(img[3::4] == 1.0)
    assert se.shape == (w * h,) and bool(torch.isfinite(se).all()) and bool((se > 0).any())
    # a target between two of the history's values: stops at the first batch at or below it
    k = 3
    target = 0.5 * (hist[k - 1] + hist[k])
    img2, se2, done2, hist2 = error.render_to_noise(sc, S, B, target, seeds.data_ptr())
    assert done2 == (k + 1) * B and done2 < S
    assert hist2 == hist[:k + 1] and hist2[-1] <= target < hist2[-2]
    img2 = img2.cpu().numpy()
    np.testing.assert_allclose(img2, plain(done2), rtol=1e-12, atol=0)
    assert np.all(img2[3::4] == 1.0)
    # a last short batch: 80 samples in batches of 32
    _, _, done3, hist3 = error.render_to_noise(sc, 80, B, 0.0, seeds.data_ptr())
    assert done3 == 80 and len(hist3) == 3
    sc.close()
