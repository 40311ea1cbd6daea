"""Per-tile adaptive sampling (ptmi/error.py render_adaptive) on the GPU.

The target calibrates itself: the first round of render_adaptive is a render of samples [0, 16) on
every tile with the automatic plan, which is bit for bit what render_moments gives, so
target = median(tile_err) / stats[2] of that render makes about half the tiles stop after one
round and the rest go on.

What is checked against independent full-frame renders: the counts' shape (constant per tile,
multiples of the batch, nested raster-ordered lists), each pixel's value (samples [0, n) of the
max_samples-spp frame over n), and the stopping rule, re-derived round by round with
error_map_reference from full-frame batch renders masked to each round's list.  A list render and a
full-frame render may group a tile's chunk sums differently (the automatic plan depends on the
number of tiles: DESIGN.md s4b, 1e-12 relative on sums of non-negative terms); the variance is a
difference of such sums, so a tile whose error is within 1e-6 relative of the round's threshold is
not asked which side it fell on."""
import numpy as np
import pytest

from ptmi import api, error, layout
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu


def _moments(torch, sc, S, b, e, seeds):
    sums = torch.empty(sc.width * sc.height * 4, dtype=torch.float64, device="cuda")
    sq = torch.empty(sc.width * sc.height, dtype=torch.float64, device="cuda")
    sc.render_moments(S, b, e, seeds.data_ptr(), sums.data_ptr(), sq.data_ptr())
    torch.cuda.synchronize()
    return sums, sq


def _tile_of_pixel(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 8) * ((w + 7) // 8) + x // 8).reshape(-1)


@pytest.mark.parametrize("kind,w,h,S", [("reference", 64, 48, 256), ("teapot", 40, 24, 64)])
def test_adaptive_render(kind, w, h, S):
    import torch
    B = 16
    sc = api.Scene(0, *scene_inputs(kind, w, h))
    npix, tiles = w * h, ((w + 7) // 8) * ((h + 7) // 8)
    seeds = torch.tensor(layout.seeds_go_float64(npix, 77), dtype=torch.float64, device="cuda")

    # the target from the frame's own first batch
    sums0, sq0 = _moments(torch, sc, S, 0, B, seeds)
    tile_err0 = torch.empty(tiles, dtype=torch.float64, device="cuda")
    stats0 = torch.empty(4, dtype=torch.float64, device="cuda")
    api.error_map(sums0.data_ptr(), sq0.data_ptr(), w, h, stats0.data_ptr(), tile_err_ptr=tile_err0.data_ptr())
    tile_err0, stats0 = tile_err0.cpu().numpy(), stats0.cpu().numpy()
    assert tile_err0.min() < tile_err0.max(), "every tile equally noisy: the scene cannot test the feature"
    target = float(np.median(tile_err0)) / float(stats0[2])

    img, se, counts, hist, lists = error.render_adaptive(sc, S, B, target, seeds.data_ptr(), keep_lists=True)
    img2, _, counts2, hist2 = error.render_adaptive(sc, S, B, target, seeds.data_ptr())
    assert torch.equal(img, img2) and torch.equal(counts, counts2) and hist == hist2  # reproducible
    img, counts = img.cpu().numpy().reshape(npix, 4), counts.cpu().numpy()
    rounds = len(hist)
    print("%s: %d rounds, active tiles per round %s" % (kind, rounds, [a for a, _, _ in hist]))

    # counts: constant per tile, multiples of the batch (or max_samples), at most max_samples
    tile_px = _tile_of_pixel(w, h)
    tile_n = np.zeros(tiles)
    for t in range(tiles):
        c = counts[tile_px == t]
        assert np.all(c == c[0])
        tile_n[t] = c[0]
    assert np.all((tile_n % B == 0) | (tile_n == S)) and tile_n.max() <= S
    assert counts.min() == B < counts.max()

    # lists: every tile first, nested, in raster order; a tile's count is what its rounds traced
    assert len(lists) == rounds and np.array_equal(lists[0], np.arange(tiles))
    traced = np.zeros(tiles)
    for r, lst in enumerate(lists):
        assert hist[r][0] == len(lst) > 0
        assert np.all(np.diff(lst.astype(np.int64)) > 0)
        if r:
            assert np.isin(lst, lists[r - 1]).all()
        traced[lst] += min((r + 1) * B, S) - r * B
    assert np.array_equal(traced, tile_n)
    # the first round is the calibration render: the tiles at or below the median stopped there
    assert hist[0][1] == target * stats0[2]
    assert np.array_equal(lists[1], np.nonzero(tile_err0 > hist[0][1])[0]) if rounds > 1 else True

    # the stopping rule, round by round, from full-frame batch renders masked to the round's list
    acc_s, acc_q = np.zeros((npix, 4)), np.zeros(npix)
    margin = 1e-6
    for r, lst in enumerate(lists):
        bs, bq = _moments(torch, sc, S, r * B, min((r + 1) * B, S), seeds)
        m = np.isin(tile_px, lst)
        acc_s[m] += bs.cpu().numpy().reshape(npix, 4)[m]
        acc_q[m] += bq.cpu().numpy()[m]
        _, terr, st = error.error_map_reference(acc_s.reshape(-1), acc_q, w, h)
        thr = hist[r][1]
        assert abs(thr - target * st[2]) <= 1e-9 * thr
        assert abs(hist[r][2] - st[0] / st[2]) <= 1e-6 * hist[r][2]
        nxt = lists[r + 1] if r + 1 < rounds else np.zeros(0, dtype=np.uint32)
        for t in lst:
            if abs(terr[t] - thr) <= margin * thr:
                continue
            if r + 1 < rounds:
                assert (t in nxt) == (terr[t] > thr), (r, t, terr[t], thr)
            elif min((r + 1) * B, S) < S:  # the loop ended because no tile was left
                assert terr[t] <= thr

    # every pixel: samples [0, n) of the S-spp frame over n
    for n in np.unique(tile_n):
        fs, _ = _moments(torch, sc, S, 0, int(n), seeds)
        fs = fs.cpu().numpy().reshape(npix, 4)
        m = counts == n
        np.testing.assert_allclose(img[m, :3], fs[m, :3] * (1.0 / n), rtol=1e-12, atol=0)
    assert np.all(img[:, 3] == 1.0)

    # against the whole-frame loop with the same target
    _, _, done, hist_u = error.render_to_noise(sc, S, B, target, seeds.data_ptr())
    print("%s: render_to_noise stopped at %d spp (%d samples, final ratio %.4g); adaptive traced %d samples "
          "(mean %.1f spp, final ratio %.4g)" % (kind, done, done * npix, hist_u[-1], int(counts.sum()),
                                                 counts.mean(), hist[-1][2]))
    if done < S:
        assert counts.sum() < npix * S
    sc.close()


def test_adaptive_arguments():
    sc = api.Scene(0, *scene_inputs("reference", 16, 16))
    with pytest.raises(ValueError):
        error.render_adaptive(sc, 64, 1, 0.1, 0)
    with pytest.raises(ValueError):
        error.render_adaptive(sc, 0, 16, 0.1, 0)
    sc.close()
