"""Per-pixel noise estimates from the moment render (ptmi_scene_render_moments, ptmi_error_map).

``error_map_reference`` is the numpy restatement of the device's error map, operation for
operation (csrc/ptmi_image_kernels.hip pixel_err / error_map / error_stats): the formula's
documentation and the comparator of the GPU tests.

``render_to_noise`` renders a frame batch by batch until its relative noise is below a target.
Sample indices are global, so the batches [0, b), [b, 2b), ... of a ``max_samples``-spp frame are
that frame, stopped early.

``render_adaptive`` stops each 8x8 tile on its own (ptmi_scene_render_tiles, ptmi_select_tiles,
ptmi_finalize_counts); ``select_tiles_reference`` and ``finalize_counts_reference`` restate the two
small kernels.
"""
import numpy as np

TILE = 8  # the kernels' 8x8 pixel tiles (csrc/ptmi_device.h kTile)


def _tree(v, op):
    """The device's fixed-shape reduction over the last axis (a power of two long): slot t takes
    op(slot t, slot t + s) for s = len/2, len/4, ..., 1."""
    v = np.array(v, dtype=np.float64)
    s = v.shape[-1] // 2
    while s > 0:
        v = op(v[..., :s], v[..., s:2 * s])
        s //= 2
    return v[..., 0]


def _summaries(se2, se_fin, mean, cnt):
    """(sum se2, max finite se, sum mean, count) of the rows' 64 slots by the device's tree."""
    return _tree(se2, np.add), _tree(se_fin, np.maximum), _tree(mean, np.add), _tree(cnt, np.add)


def error_map_reference(sums, sq, width, height):
    """(se[H*W], tile_err[tiles], stats[4]) from frame sums (W*H*4: r, g, b, n) and second moments.

    Per pixel, n = sums[4i+3]:
        n == 0: se = 0 (not owned);  n == 1: se = +inf;  otherwise
        mean_c = sum_c / n
        d   = sq / n - ((mean_r*mean_r + mean_g*mean_g) + mean_b*mean_b)
        var = max(d, 0) * (n / (n - 1));  se2 = var / n;  se = sqrt(se2)
    se is the standard error of the pixel's mean, the root of the three channels' summed
    variances.  The summaries run over the pixels with n >= 2 and add se2 itself:
        tile_err[t] = sqrt(sum se2 / count) per 8x8 tile in raster order, 0 for an empty tile
        stats = (sqrt(sum se2 / count), largest finite se, sum(((mean_r + mean_g) + mean_b) / 3) / count, count)
    """
    w, h = int(width), int(height)
    s = np.asarray(sums, dtype=np.float64).reshape(h * w, 4)
    q = np.asarray(sq, dtype=np.float64).reshape(h * w)
    n = s[:, 3]
    counted = ~((n == 0.0) | (n == 1.0))
    with np.errstate(all="ignore"):
        nn = np.where(counted, n, 2.0)
        mr, mg, mb = s[:, 0] / nn, s[:, 1] / nn, s[:, 2] / nn
        d = q / nn - ((mr * mr + mg * mg) + mb * mb)
        var = np.where(d < 0.0, 0.0, d) * (nn / (nn - 1.0))
        se2 = np.where(counted, var / nn, 0.0)
        se = np.where(counted, np.sqrt(se2), np.where(n == 1.0, np.inf, 0.0))
        mean = np.where(counted, ((mr + mg) + mb) / 3.0, 0.0)
    se_fin = np.where(counted & (se < np.inf), se, 0.0)  # (a NaN se compares false)
    # the tiles' 64 slots, lane = (y & 7) * 8 + (x & 7); slots outside the image hold zeros
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE

    def tiled(a):
        full = np.zeros((ty * TILE, tx * TILE))
        full[:h, :w] = a.reshape(h, w)
        return full.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty * tx, TILE * TILE)

    with np.errstate(all="ignore"):
        t_se2, t_max, t_mean, t_cnt = _summaries(tiled(se2), tiled(se_fin), tiled(mean), tiled(counted.astype(np.float64)))
        tile_err = np.where(t_cnt > 0.0, np.sqrt(t_se2 / np.where(t_cnt > 0.0, t_cnt, 1.0)), 0.0)
        # the frame: thread t of 256 folds tiles t, t + 256, ... in that order, then the tree
        tiles = tx * ty
        rows = (tiles + 255) // 256
        acc = np.zeros((4, 256))
        for r in range(rows):
            k = slice(r * 256, min((r + 1) * 256, tiles))
            m = k.stop - k.start
            acc[0, :m] = acc[0, :m] + t_se2[k]
            acc[1, :m] = np.where(t_max[k] > acc[1, :m], t_max[k], acc[1, :m])
            acc[2, :m] = acc[2, :m] + t_mean[k]
            acc[3, :m] = acc[3, :m] + t_cnt[k]
        f_se2, f_mean, f_cnt = _tree(acc[0], np.add), _tree(acc[2], np.add), _tree(acc[3], np.add)
        f_max = _tree(acc[1], lambda a, b: np.where(b > a, b, a))
        stats = np.array([np.sqrt(f_se2 / f_cnt) if f_cnt > 0 else 0.0, f_max, f_mean / f_cnt if f_cnt > 0 else 0.0,
                          f_cnt])
    return se, tile_err, stats


def select_tiles_reference(tile_err, in_tiles, n_in, threshold):
    """(kept tiles as uint32, their number): of the candidates in_tiles[0..n_in) -- the tiles 0..n_in
    themselves when in_tiles is None -- those with tile_err[t] > threshold, in candidate order.  A
    NaN error and an error equal to the threshold are dropped, +inf is kept (ptmi_select_tiles)."""
    err = np.asarray(tile_err, dtype=np.float64)
    n_in = int(n_in)
    cand = np.arange(n_in, dtype=np.uint32) if in_tiles is None else np.asarray(in_tiles, dtype=np.uint32)[:n_in]
    with np.errstate(invalid="ignore"):
        keep = err[cand.astype(np.int64)] > np.float64(threshold) if n_in else np.zeros(0, dtype=bool)
    out = cand[keep]
    return out, int(out.size)


def finalize_counts_reference(sums):
    """RGBA (n_pixels * 4) from frame sums (r, g, b, n per pixel) by each pixel's own count:
    RGB = sum_c * (1.0 / n), 0 where n == 0; A = 1.0 (ptmi_finalize_counts)."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 4)
    n = s[:, 3]
    with np.errstate(all="ignore"):
        w = 1.0 / n
        out = np.where((n == 0.0)[:, None], 0.0, s * w[:, None])
    out[:, 3] = 1.0
    return out.reshape(-1)


def render_to_noise(scene, max_samples, batch, target, seeds_ptr, chunks=0, stream=None, denoise=False,
                    denoise_params=None, guides="first"):
    """Render `scene` (api.Scene) until the frame's relative noise is at most `target`.

    Batches [k*batch, (k+1)*batch) of a `max_samples`-spp frame (the last one short if needed) are
    rendered with render_moments and accumulated; after each, error_map gives stats, and the loop
    stops after the first batch with stats[0] <= target * stats[2] -- rms standard error of the
    pixel means against the mean pixel value -- or when the samples run out.  The frame is
    finalised with the number of samples done.

    Returns (image, se, samples_done, history): float64 torch tensors on the scene's device, RGBA
    of W*H*4 and the standard-error map of W*H, and the per-batch stats[0] / stats[2].  With `denoise`
    the image and the map are the filtered ones (ptmi/denoise.py denoise_frame, `denoise_params`, and
    `guides`: "first" or "specular").
    """
    import torch
    from . import api

    if max_samples <= 0 or batch <= 0:
        raise ValueError("max_samples and batch must be positive")
    npix = scene.width * scene.height
    st = torch.cuda.current_stream() if stream is None else stream
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        kw = dict(dtype=torch.float64, device="cuda")
        sums, sq = torch.zeros(npix * 4, **kw), torch.zeros(npix, **kw)
        b_sums, b_sq = torch.empty(npix * 4, **kw), torch.empty(npix, **kw)
        se, stats, out = torch.empty(npix, **kw), torch.empty(4, **kw), torch.empty(npix * 4, **kw)
        history, done = [], 0
        while done < max_samples:
            end = min(done + batch, max_samples)
            scene.render_moments(max_samples, done, end, seeds_ptr, b_sums.data_ptr(), b_sq.data_ptr(),
                                 chunks=chunks, stream=sp)
            api.accumulate(sums.data_ptr(), b_sums.data_ptr(), npix * 4, stream=sp)
            api.accumulate(sq.data_ptr(), b_sq.data_ptr(), npix, stream=sp)
            api.error_map(sums.data_ptr(), sq.data_ptr(), scene.width, scene.height, stats.data_ptr(),
                          se_ptr=se.data_ptr(), stream=sp)
            done = end
            rms, _, mean, _ = stats.tolist()  # (waits for the batch)
            history.append(rms / mean if mean != 0.0 else float("inf"))
            if rms <= target * mean:
                break
        scene.finalize(sums.data_ptr(), out.data_ptr(), done, stream=sp)
        if denoise:
            from .denoise import denoise_frame
            out, se, _ = denoise_frame(scene, out, se, params=denoise_params, stream=st, guides=guides)
    return out, se, done, history


def render_adaptive(scene, max_samples, batch, target, seeds_ptr, chunks=0, stream=None, keep_lists=False,
                    denoise=False, denoise_params=None, guides="first"):
    """Render `scene` (api.Scene) with each 8x8 tile stopping on its own noise.

    Round r traces samples [r*batch, (r+1)*batch) of a `max_samples`-spp frame (the last round short
    if needed) on the active tiles only (render_tiles), accumulates them, and takes tile_err and stats
    from error_map over the whole frame.  A tile stays active while tile_err > threshold, with
    threshold = target * stats[2] of that round (select_tiles, from the active list into the other of
    two buffers, so the lists are nested and stay in raster order).  The loop ends when no tile is
    active or the samples run out.  The active set only shrinks, so a pixel with count n holds exactly
    samples [0, n) of the frame; the image divides each pixel by its own count (finalize_counts).

    What a stopped tile is promised: its tile_err was <= the threshold of the round it stopped in.
    The threshold follows stats[2] from round to round, so the final frame ratio stats[0] / stats[2]
    (the last history entry) is reported, not guaranteed.  Stopping on the sample variance makes the
    estimate slightly biased (pixels whose first samples happen to agree stop early): a property of
    the method.  Each round waits for the device twice, for stats and for the new list's length.

    `batch` >= 2 (one sample has no variance).  Returns (image, se, counts, history): float64 torch
    tensors on the scene's device -- RGBA of W*H*4, the standard-error map and the per-pixel sample
    counts of W*H -- and one (active tiles, threshold, stats[0] / stats[2]) per round.  With
    keep_lists a fifth element: each round's active list, numpy uint32 arrays.  With `denoise` the image
    and the map are the filtered ones (ptmi/denoise.py denoise_frame, `denoise_params`, and `guides`:
    "first" or "specular"); the stopping rule does not see the filter.
    """
    import torch
    from . import api

    if max_samples <= 0 or batch < 2:
        raise ValueError("max_samples must be positive and batch at least 2")
    w, h = scene.width, scene.height
    npix = w * h
    tiles = ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)
    st = torch.cuda.current_stream() if stream is None else stream
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        kw = dict(dtype=torch.float64, device="cuda")
        sums, sq = torch.zeros(npix * 4, **kw), torch.zeros(npix, **kw)
        b_sums, b_sq = torch.empty(npix * 4, **kw), torch.empty(npix, **kw)
        se, stats, out = torch.empty(npix, **kw), torch.empty(4, **kw), torch.empty(npix * 4, **kw)
        tile_err = torch.empty(tiles, **kw)
        cur = torch.arange(tiles, dtype=torch.int32, device="cuda")  # (uint32 on the device side)
        nxt, count = torch.empty_like(cur), torch.zeros(1, dtype=torch.int32, device="cuda")
        history, lists, done, active = [], [], 0, tiles
        while True:
            end = min(done + batch, max_samples)
            if keep_lists:
                lists.append(cur[:active].cpu().numpy().astype(np.uint32))
            scene.render_tiles(max_samples, done, end, cur.data_ptr(), active, seeds_ptr, b_sums.data_ptr(),
                               b_sq.data_ptr(), chunks=chunks, stream=sp)
            api.accumulate(sums.data_ptr(), b_sums.data_ptr(), npix * 4, stream=sp)
            api.accumulate(sq.data_ptr(), b_sq.data_ptr(), npix, stream=sp)
            api.error_map(sums.data_ptr(), sq.data_ptr(), w, h, stats.data_ptr(), se_ptr=se.data_ptr(),
                          tile_err_ptr=tile_err.data_ptr(), stream=sp)
            done = end
            rms, _, mean, _ = stats.tolist()  # (waits for the round)
            threshold = target * mean
            history.append((active, threshold, rms / mean if mean != 0.0 else float("inf")))
            api.select_tiles(tile_err.data_ptr(), cur.data_ptr(), active, threshold, nxt.data_ptr(),
                             count.data_ptr(), stream=sp)
            active = int(count.item())  # (waits for the list)
            cur, nxt = nxt, cur
            if active == 0 or done == max_samples:
                break
        counts = sums[3::4].clone()
        scene.finalize_counts(sums.data_ptr(), out.data_ptr(), stream=sp)
        if denoise:
            from .denoise import denoise_frame
            out, se, _ = denoise_frame(scene, out, se, params=denoise_params, stream=st, guides=guides)
    return (out, se, counts, history, lists) if keep_lists else (out, se, counts, history)
