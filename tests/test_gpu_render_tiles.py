"""ptmi_scene_render_tiles (a moment render on a caller's list of 8x8 tiles) against
ptmi_scene_render_moments of the whole frame.

With the same explicit chunk count both launches cut every tile's samples alike, so a listed tile's
sums and second moments must equal the full frame's bit for bit, whichever kernel family traces the
scene, and every other pixel must be exactly 0.  With chunks = 0 the plan depends on how many tiles
the launch owns, so the sums may be regrouped: equal within 1e-12 relative (all terms
are non-negative), and two such calls equal each other bit for bit.

The frame is 44x27: 6x4 tiles with edge tiles on both axes, so lanes outside the image are in the
listed corner tile 23.  The teapot frames hold fewer tiles and have their own lists.  The wide-code
mesh (F_WIDE) is not here, as in tests/test_gpu_moments.py: its scene helper alone takes ~10 s; its
moment instantiations take the same wave-uniform select as the other families without list forms
(ptmi_kernels.hip kTilesOf), covered by inspection.
"""
import numpy as np
import pytest

from ptmi import api, layout
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu

W, H = 44, 27
LIST = [23, 0, 7, 14]  # unordered; 23 is the corner edge tile


def _scene(kind, w, h):
    """-> api.Scene for the case's kernel family (the helpers of tests/test_gpu_moments.py)."""
    if kind == "reference_dof":
        return api.Scene(0, *scene_inputs("reference", w, h, 0.15, 1.6))
    if kind == "textures":  # F_ALL | F_PROJ | F_TEX
        from tests import textures_synth
        return api.Scene(0, *scene_inputs("textures", w, h), *textures_synth.scene_textures("textures"))
    if kind == "teapot_generic":  # a mesh through the generic instantiation (trace_groups, no pool)
        with api.force_flags(31):
            return api.Scene(0, *scene_inputs("teapot", w, h))
    return api.Scene(0, *scene_inputs(kind, w, h))


def _tile_mask(w, h, tiles):
    """bool[h * w]: the pixels of the listed tiles (raster indices; out-of-range entries own nothing)."""
    tx = (w + 7) // 8
    ty = (h + 7) // 8
    m = np.zeros((h, w), dtype=bool)
    for t in tiles:
        if 0 <= t < tx * ty:
            m[(t // tx) * 8:(t // tx) * 8 + 8, (t % tx) * 8:(t % tx) * 8 + 8] = True
    return m.reshape(-1)


class _Run:
    def __init__(self, kind, w, h, S, seed=33, rng=None):
        import torch
        self.torch, self.w, self.h, self.S, self.n = torch, w, h, S, w * h
        self.sc = _scene(kind, w, h)
        if rng is not None:
            self.sc.set_rng(rng)
        self.seeds = torch.tensor(layout.seeds_go_float64(self.n, seed), dtype=torch.float64, device="cuda")
        self._full = {}

    def _bufs(self):
        t = self.torch
        return (t.full((self.n * 4,), -1.0, dtype=t.float64, device="cuda"),
                t.full((self.n,), -1.0, dtype=t.float64, device="cuda"))

    def full(self, b, e, **kw):
        """The full-frame moment render, computed once per argument set."""
        key = (b, e, tuple(sorted(kw.items())))
        if key not in self._full:
            sums, sq = self._bufs()
            self.sc.render_moments(self.S, b, e, self.seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), **kw)
            self.torch.cuda.synchronize()
            self._full[key] = (sums.cpu().numpy(), sq.cpu().numpy())
        return self._full[key]

    def tiles(self, b, e, tiles, n_tiles=None, chunks=0):
        t = self.torch
        lst = t.tensor(np.asarray(tiles, dtype=np.uint32).view(np.int32), dtype=t.int32, device="cuda")
        sums, sq = self._bufs()
        self.sc.render_tiles(self.S, b, e, lst.data_ptr() if len(tiles) else 0,
                             len(tiles) if n_tiles is None else n_tiles, self.seeds.data_ptr(), sums.data_ptr(),
                             sq.data_ptr(), chunks=chunks)
        t.cuda.synchronize()
        return sums.cpu().numpy(), sq.cpu().numpy()

    def check_exact(self, b, e, tiles, chunks):
        """Listed tiles bit-equal to the full frame's, every other pixel exactly 0."""
        fs, fq = self.full(b, e, chunks=chunks)
        sums, sq = self.tiles(b, e, tiles, chunks=chunks)
        m = _tile_mask(self.w, self.h, tiles)
        assert m.any() and not m.all()
        sums, fs = sums.reshape(-1, 4), fs.reshape(-1, 4)
        assert np.all(sums[m, 3] == e - b)
        assert np.array_equal(sums[m], fs[m], equal_nan=True), "listed tiles' sums differ from the full frame's"
        assert np.array_equal(sq[m], fq[m], equal_nan=True), "listed tiles' second moments differ"
        assert np.all(sums[~m] == 0) and np.all(sq[~m] == 0)
        assert not np.signbit(sums[~m]).any() and not np.signbit(sq[~m]).any()

    def close(self):
        self.sc.close()


def _family(kind, w, h, S, tiles, b=0, rng=None):
    r = _Run(kind, w, h, S, rng=rng)
    for chunks in (1, 3):
        r.check_exact(b, S, tiles, chunks)
    return r


def test_reference_scene_lockstep_family():
    r = _family("reference", W, H, 32, LIST)
    assert not r.sc.kernel_flags() & (1 | 4 | 8 | 16 | 32)  # the lockstep kernels: <512>'s select
    r.check_exact(5, 29, LIST, 2)  # a sub-range of the samples
    r.close()


def test_reference_scene_dof_family():
    """Sample 0 of a DoF frame (the NaN ray, contribution 0) is in the range."""
    r = _family("reference_dof", W, H, 32, LIST)
    assert r.sc.kernel_flags() & 8 and not r.sc.kernel_flags() & (1 | 4)  # F_DOF, lockstep: <520>
    r.close()


def test_ocl_scene_materials_family():
    r = _family("default", W, H, 32, LIST)
    assert r.sc.kernel_flags() & 4 and not r.sc.kernel_flags() & 1  # F_MATERIALS, no mesh
    r.close()


def test_teapot_pooled_mesh_family():
    """40x24: 5x3 tiles, through the F_TLIST | F_MOM instantiations with the caller's list."""
    r = _family("teapot", 40, 24, 32, [14, 0, 7, 11])
    assert r.sc.kernel_flags() & 1 and not r.sc.kernel_flags() & (16 | 32 | 64)  # the path pool's kernels
    r.close()


def test_teapot_generic_family():
    r = _family("teapot_generic", 40, 24, 32, [14, 0, 7, 11])
    assert r.sc.kernel_flags() & 16 and r.sc.kernel_flags() & 1  # F_PROJ with a mesh: trace_groups
    r.close()


def test_statistical_rng_family():
    r = _family("reference", W, H, 32, LIST, rng=api.RNG_XOSHIRO)
    assert r.sc.kernel_flags() & 64
    r.close()


def test_textured_family():
    r = _family("textures", W, H, 32, LIST)
    assert r.sc.kernel_flags() & 32  # F_TEX
    r.close()


@pytest.mark.parametrize("kind,w,h,tiles", [("reference", W, H, LIST), ("teapot", 40, 24, [14, 0, 7, 11])])
def test_automatic_plan_is_reproducible_and_within_regrouping(kind, w, h, tiles):
    r = _Run(kind, w, h, 64)
    fs, fq = r.full(0, 64, chunks=0)
    s1, q1 = r.tiles(0, 64, tiles, chunks=0)
    s2, q2 = r.tiles(0, 64, tiles, chunks=0)
    assert np.array_equal(s1, s2, equal_nan=True) and np.array_equal(q1, q2, equal_nan=True)
    m = _tile_mask(w, h, tiles)
    m4 = np.repeat(m, 4)
    print("max rel. difference: sums %.3e sq %.3e" % (
        np.max(np.abs(s1[m4] - fs[m4]) / np.where(fs[m4] != 0, np.abs(fs[m4]), 1.0)),
        np.max(np.abs(q1[m] - fq[m]) / np.where(fq[m] != 0, np.abs(fq[m]), 1.0))))
    np.testing.assert_allclose(s1[m4], fs[m4], rtol=1e-12, atol=0)
    np.testing.assert_allclose(q1[m], fq[m], rtol=1e-12, atol=0)
    assert not s1[~m4].any() and not q1[~m].any()
    r.close()


def test_boundary_cases():
    r = _Run("reference", W, H, 32)
    n_tiles = 6 * 4
    for chunks in (1, 3):
        fs, fq = r.full(0, 32, chunks=chunks)
        # no tile: all zeros, with and without a list pointer
        sums, sq = r.tiles(0, 32, [], chunks=chunks)
        assert not sums.any() and not sq.any()
        sums, sq = r.tiles(0, 32, [3], n_tiles=0, chunks=chunks)
        assert not sums.any() and not sq.any()
        # every tile in raster order: the full moment render
        sums, sq = r.tiles(0, 32, list(range(n_tiles)), chunks=chunks)
        assert np.array_equal(sums, fs) and np.array_equal(sq, fq)
        # out-of-range entries are skipped (the first past the end, a large one, the largest)
        bad = [3, n_tiles, 5, 100000, 0xFFFFFFFF, 22]
        sums, sq = r.tiles(0, 32, bad, chunks=chunks)
        m = _tile_mask(W, H, [3, 5, 22])
        m4 = np.repeat(m, 4)
        assert np.array_equal(sums[m4], fs[m4]) and np.array_equal(sq[m], fq[m])
        assert not sums[~m4].any() and not sq[~m].any()
    # a NULL list with tiles to render is refused, and nothing is written
    t = r.torch
    sums, sq = r._bufs()
    with pytest.raises(api.PtmiError) as e:
        r.sc.render_tiles(32, 0, 32, 0, 4, r.seeds.data_ptr(), sums.data_ptr(), sq.data_ptr())
    assert e.value.code == api.PTMI_ERR_ARG
    with pytest.raises(api.PtmiError) as e:  # sq is required
        r.sc.render_tiles(32, 0, 32, r.seeds.data_ptr(), 0, r.seeds.data_ptr(), sums.data_ptr(), 0)
    assert e.value.code == api.PTMI_ERR_ARG
    t.cuda.synchronize()
    assert t.all(sums == -1.0).item() and t.all(sq == -1.0).item()
    r.close()


def test_tile_split_render_survives_a_list_render():
    """Teapot 32x20 (4 tiles per row: diagonal ownership through the library's cached tile list and
    its cached dispatch order): a tile-split moment render issued after a render_tiles call equals
    the one issued before it."""
    r = _Run("teapot", 32, 20, 24)
    assert r.sc.tile_ownership(2) == "diagonal"

    def shard(g):
        sums, sq = r._bufs()
        r.sc.render_moments(24, 0, 24, r.seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), tile_stride=2,
                            tile_offset=g)
        r.torch.cuda.synchronize()
        return sums.cpu().numpy(), sq.cpu().numpy()

    before = shard(1)
    r.check_exact(0, 24, [11, 2, 5], 2)
    r.tiles(0, 24, [11, 2, 5], chunks=0)
    after = shard(1)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    other = shard(0)  # (and the cache still follows a change of the offset)
    fs, fq = r.full(0, 24, chunks=0)
    np.testing.assert_allclose(after[1] + other[1], fq, rtol=1e-12, atol=0)
    r.close()
