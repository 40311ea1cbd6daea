"""Per-pixel second moments (ptmi_scene_render_moments) against the plain entry point.

ptmi_scene_render(S, n, n + 1) returns sample n's path colour per pixel, so the expected second
moment is m2 = sum_n ((r_n^2 + g_n^2) + b_n^2), formed in numpy from one-sample renders.  Every term
is non-negative, so another order of the adds moves m2 by at most ~S * 2^-53 relative: rtol 1e-12
everywhere, and bit-equality where the kernel adds a pixel's paths in sample order (one chunk, the
kernels without the path pool).  In every case the moment render's colour sums are the plain
render's bit for bit and a second moment render repeats the first bit for bit.

Frames are no multiple of 8 wide or high: edge tiles are in every case.  The wide-code mesh
(F_WIDE) is not here: its scene helper alone takes ~10 s (covered by inspection).
"""
import numpy as np
import pytest

from ptmi import api, layout
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu


def _scene(kind, w, h):
    """-> api.Scene for the case's kernel family."""
    if kind == "reference_dof":
        return api.Scene(0, *scene_inputs("reference", w, h, 0.15, 1.6))
    if kind == "textures":  # F_ALL | F_PROJ | F_TEX
        from tests import textures_synth
        return api.Scene(0, *scene_inputs("textures", w, h), *textures_synth.scene_textures("textures"))
    if kind == "nonaffine":  # a sphere scaled by 2^-70 is outside the tame-scene bound: F_ALL | F_PROJ
        from ptmi import geom, scenes, shapes
        ref = scenes.reference_scene(w, h)
        tiny = shapes.Sphere()
        tiny.set_transform(geom.translate(0.1, 0.1, -0.2))
        tiny.set_transform(geom.scale(2.0 ** -70, 2.0 ** -70, 2.0 ** -70))
        tiny.set_material(shapes.new_diffuse(0.5, 0.5, 0.5))
        objs, tris, grps = layout.build_scene_buffer_cl(ref.objects + [tiny])
        return api.Scene(0, objs, tris, grps, layout.camera_record(ref.camera))
    if kind == "teapot_generic":  # a mesh through the generic instantiation (trace_groups, no pool)
        with api.force_flags(31):
            return api.Scene(0, *scene_inputs("teapot", w, h))
    return api.Scene(0, *scene_inputs(kind, w, h))


class _Run:
    def __init__(self, kind, w, h, S, seed=21, rng=None):
        import torch
        self.torch, self.w, self.h, self.S, self.n = torch, w, h, S, w * h
        self.sc = _scene(kind, w, h)
        if rng is not None:
            self.sc.set_rng(rng)
        self.seeds = torch.tensor(layout.seeds_go_float64(self.n, seed), dtype=torch.float64, device="cuda")
        self._paths = {}

    def plain(self, b, e, **kw):
        out = self.torch.empty(self.n * 4, dtype=self.torch.float64, device="cuda")
        self.sc.render(self.S, b, e, self.seeds.data_ptr(), out.data_ptr(), **kw)
        self.torch.cuda.synchronize()
        return out.cpu().numpy()

    def moments(self, b, e, **kw):
        t = self.torch
        sums = t.full((self.n * 4,), -1.0, dtype=t.float64, device="cuda")
        sq = t.full((self.n,), -1.0, dtype=t.float64, device="cuda")
        self.sc.render_moments(self.S, b, e, self.seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), **kw)
        t.cuda.synchronize()
        return sums.cpu().numpy(), sq.cpu().numpy()

    def expected(self, b, e, stride=1, offset=0):
        """m2 from one-sample renders of the plain entry point, added in sample order."""
        m2 = np.zeros(self.n)
        for n in range(b, e):
            key = (n, stride, offset)
            if key not in self._paths:
                self._paths[key] = self.plain(n, n + 1, tile_stride=stride, tile_offset=offset).reshape(-1, 4)
            p = self._paths[key]
            m2 = m2 + ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        return m2

    def check(self, b, e, exact, **kw):
        """The three properties of a moment render; returns (sums, sq)."""
        plain = self.plain(b, e, **kw)
        sums, sq = self.moments(b, e, **kw)
        sums2, sq2 = self.moments(b, e, **kw)
        assert np.array_equal(sums, plain, equal_nan=True), "colour sums differ from ptmi_scene_render's"
        assert np.array_equal(sq, sq2, equal_nan=True) and np.array_equal(sums, sums2, equal_nan=True)
        exp = self.expected(b, e, kw.get("tile_stride", 1), kw.get("tile_offset", 0))
        with np.errstate(all="ignore"):
            rel = np.nanmax(np.abs(sq - exp) / np.where(exp > 0, exp, 1.0))
        print("m2 max rel. difference %.3e, equal bits: %s" % (rel, np.array_equal(sq, exp, equal_nan=True)))
        np.testing.assert_allclose(sq, exp, rtol=1e-12, atol=0, equal_nan=True)
        if exact:
            assert np.array_equal(sq, exp, equal_nan=True), "sample-order sums must equal bit for bit"
        return sums, sq

    def close(self):
        self.sc.close()


def test_reference_scene_lockstep_family():
    r = _Run("reference", 36, 20, 13)
    assert not r.sc.kernel_flags() & (1 | 4 | 8 | 16 | 32)  # the lockstep kernels
    r.check(0, 13, True, chunks=1)
    r.check(0, 13, False, chunks=3)  # 5 + 5 + 3 samples: the partial planes and reduce_chunks_kernel<true>
    r.check(0, 13, False, chunks=0)
    r.close()


def test_reference_scene_dof_nan_ray_adds_zero():
    """Sample 0 of a DoF frame is the reference's NaN ray, which ptmi ends with contribution 0."""
    r = _Run("reference_dof", 20, 12, 9)
    assert r.sc.kernel_flags() & 8 and not r.sc.kernel_flags() & (1 | 4)  # F_DOF, lockstep
    sums0, sq0 = r.moments(0, 1, chunks=1)
    assert np.all(sums0.reshape(-1, 4)[:, :3] == 0) and np.all(sums0[3::4] == 1)
    assert np.all(sq0 == 0) and not np.signbit(sq0).any()
    r.check(0, 9, True, chunks=1)
    r.check(0, 9, False, chunks=2)
    r.close()


def test_ocl_scene_materials_family():
    r = _Run("default", 36, 20, 13)  # cylinder, cube, glass, mirror
    assert r.sc.kernel_flags() & 4 and not r.sc.kernel_flags() & 1  # F_MATERIALS, no mesh
    r.check(0, 13, True, chunks=1)
    r.check(0, 13, False, chunks=3)
    r.close()


def test_teapot_pooled_mesh_family():
    r = _Run("teapot", 28, 20, 24)
    assert r.sc.kernel_flags() & 1 and not r.sc.kernel_flags() & (16 | 32 | 64)  # the path pool's kernels
    r.check(0, 24, False, chunks=0)
    r.check(0, 24, False, chunks=2)
    r.check(5, 19, False, chunks=0)
    r.close()


@pytest.mark.parametrize("kind,flags", [("nonaffine", 16), ("textures", 32), ("teapot_generic", 16)])
def test_generic_instantiations(kind, flags):
    r = _Run(kind, 20, 12, 8)
    assert r.sc.kernel_flags() & flags  # F_PROJ / F_TEX
    r.check(0, 8, True, chunks=1)
    r.check(0, 8, False, chunks=3)
    r.close()


@pytest.mark.parametrize("kind,w,h", [("reference", 36, 20), ("teapot", 28, 20)])
def test_statistical_rng(kind, w, h):
    """xoshiro streams are per (pixel, sample): deterministic and split-independent, so the
    one-sample reference holds; these mesh kernels (trace_groups) sum in sample order."""
    r = _Run(kind, w, h, 13, rng=api.RNG_XOSHIRO)
    assert r.sc.kernel_flags() & 64
    r.check(0, 13, True, chunks=1)
    r.check(0, 13, False, chunks=3)
    r.close()


@pytest.mark.parametrize("kind,w,h,S", [("teapot", 32, 20, 24), ("reference", 36, 20, 13)])
def test_tile_split(kind, w, h, S):
    """Two tile shards (teapot, 4 tiles per row: the F_TLIST kernels' diagonal ownership): sq is 0
    exactly where a shard owns nothing, and the shards add up to the frame -- bit for bit, since
    with the same explicit chunk count every launch cuts each tile alike."""
    from ptmi import dist as pdist
    r = _Run(kind, w, h, S)
    diag = r.sc.tile_ownership(2) == "diagonal"
    assert diag == (kind == "teapot")
    _, full = r.check(0, S, False, chunks=2)
    acc = np.zeros_like(full)
    for g in (0, 1):
        sums, sq = r.check(0, S, False, chunks=2, tile_stride=2, tile_offset=g)
        mask = pdist.tile_owner_mask(w, h, 2, g, diag).reshape(-1)
        assert np.all(sq[~mask] == 0) and not np.signbit(sq[~mask]).any()
        assert np.all(sums.reshape(-1, 4)[mask, 3] == S)
        acc += sq
    assert np.array_equal(acc, full)
    r.close()


@pytest.mark.parametrize("kind,w,h", [("reference", 36, 20), ("teapot", 28, 20)])
def test_sample_split(kind, w, h):
    r = _Run(kind, w, h, 13)
    _, a = r.moments(0, 7)
    _, b = r.moments(7, 13)
    _, full = r.moments(0, 13)
    np.testing.assert_allclose(a + b, full, rtol=1e-12, atol=0)
    r.close()


def test_pooled_item_guard():
    """A pooled work item numbers its paths 64 x samples in 32 bits: one chunk over 2^26 samples is
    refused before anything is launched (the plain entry point guards only tile-list launches)."""
    r = _Run("teapot", 28, 20, 1 << 26)
    t = r.torch
    sums = t.zeros(r.n * 4, dtype=t.float64, device="cuda")
    sq = t.zeros(r.n, dtype=t.float64, device="cuda")
    with pytest.raises(api.PtmiError) as e:
        r.sc.render_moments(1 << 26, 0, 1 << 26, r.seeds.data_ptr(), sums.data_ptr(), sq.data_ptr(), chunks=1)
    assert e.value.code == api.PTMI_ERR_ARG
    t.cuda.synchronize()
    assert not sums.any().item() and not sq.any().item()  # nothing ran
    with pytest.raises(api.PtmiError) as e:
        r.sc.render_moments(4, 0, 4, r.seeds.data_ptr(), sums.data_ptr(), 0)
    assert e.value.code == api.PTMI_ERR_ARG
    r.close()
