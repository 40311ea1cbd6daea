"""The lockstep item loop of the all-diffuse kernels without meshes (ptmi_kernels.hip
trace_lockstep) against a kernel that keeps the regeneration loop and the full
shading on every bounce.

The comparator is the material instantiation of the same scene, api.force_flags(4) (12 with
DoF): on a scene without materials it traces the same paths with the same arithmetic
(test_gpu_parity.test_generic_instantiation_matches), but through trace_kernel's regeneration
loop and bounce_shade without the dead-tail cut.  Every test first asserts which instantiation
each scene launches, so no kernel is compared with itself, and that the image is not all zeros.
Comparison is np.array_equal: a path's dead tail is never read, so nothing may
move at all.
"""
import numpy as np
import pytest

from ptmi import api, layout
from tests.scene_inputs import scene_inputs

pytestmark = pytest.mark.gpu

F_MATERIALS, F_DOF, F_XRNG = 4, 8, 64


def _scenes(w, h, ap=0.0, rng=None):
    """(lockstep scene, forced material-kernel scene) of the reference scene, flags checked."""
    objs, tris, grps, cam = scene_inputs("reference", w, h, ap, 1.6 if ap else 0.0)
    own = (F_DOF if ap else 0) | (F_XRNG if rng == api.RNG_XOSHIRO else 0)
    new = api.Scene(0, objs, tris, grps, cam)
    with api.force_flags((F_DOF if ap else 0) | F_MATERIALS):
        old = api.Scene(0, objs, tris, grps, cam)
    if rng is not None:
        new.set_rng(rng)
        old.set_rng(rng)
    assert new.kernel_flags() == own, new.kernel_flags()
    assert old.kernel_flags() == (own | F_MATERIALS), old.kernel_flags()
    return new, old


def _sums(sc, torch, seeds, spp, s0, s1, **kw):
    out = torch.empty(sc.width * sc.height * 4, dtype=torch.float64, device="cuda")
    sc.render(spp, s0, s1, seeds.data_ptr(), out.data_ptr(), **kw)
    return out


def _seeds(torch, w, h, seed):
    return torch.tensor(layout.seeds_go_float64(w * h, seed), dtype=torch.float64, device="cuda")


def _frames(w, h, spp, seed, ap=0.0, rng=None):
    import torch
    new, old = _scenes(w, h, ap, rng)
    sd = _seeds(torch, w, h, seed)
    a, b = _sums(new, torch, sd, spp, 0, spp), _sums(old, torch, sd, spp, 0, spp)
    torch.cuda.synchronize()
    new.close()
    old.close()
    return a.cpu().numpy(), b.cpu().numpy()


def _check(a, b, w, h, spp):
    assert np.any(a.reshape(-1, 4)[:, :3] != 0.0), "all-zero image"
    assert np.all(a[3::4] == spp) and a.size == w * h * 4
    assert np.array_equal(a, b), "L-inf %.3e, %d values differ" % (np.abs(a - b).max(), int((a != b).sum()))


@pytest.mark.parametrize("ap", [0.0, 0.15])
def test_lockstep_whole_tiles(ap):
    """40x24, 64 spp: whole-tile items and every path length -- the light seen directly (b == 0),
    reached at b = 1..3, escapes through the open front; with DoF, sample 0 is the NaN ray."""
    w, h, spp = 40, 24, 64
    a, b = _frames(w, h, spp, 77, ap)
    _check(a, b, w, h, spp)


def test_lockstep_edge_tiles_odd_samples():
    """37x21, 33 spp: the edge tiles hold lanes outside the image, which must stay idle."""
    w, h, spp = 37, 21, 33
    a, b = _frames(w, h, spp, 77)
    _check(a, b, w, h, spp)


def test_lockstep_chunked_tail_and_sample_shards():
    """Tail items that start at c0 != 0 (KNOB_TAIL_TILES = 5, 96 spp) and the sample shards
    [0, 17), [17, 18), [18, 96) summed in order, against the forced kernel rendering the same."""
    import torch
    w, h, spp = 40, 24, 96
    new, old = _scenes(w, h)
    sd = _seeds(torch, w, h, 77)
    res = []
    for sc in (new, old):
        assert sc.set_knob(api.KNOB_TAIL_TILES, 5) == api.PTMI_OK
        full = _sums(sc, torch, sd, spp, 0, spp)
        acc = torch.zeros_like(full)
        for s0, s1 in ((0, 17), (17, 18), (18, 96)):
            acc += _sums(sc, torch, sd, spp, s0, s1)
        torch.cuda.synchronize()
        res.append((full.cpu().numpy(), acc.cpu().numpy()))
        sc.close()
    _check(res[0][0], res[1][0], w, h, spp)
    _check(res[0][1], res[1][1], w, h, spp)


def test_lockstep_every_path():
    """One-sample renders of every n in [0, 24) (test_gpu_parity._paths): every path bit-identical,
    not only the sums."""
    import torch
    w, h, spp = 40, 24, 24
    new, old = _scenes(w, h)
    sd = _seeds(torch, w, h, 77)
    a = torch.stack([_sums(new, torch, sd, spp, n, n + 1) for n in range(spp)])
    b = torch.stack([_sums(old, torch, sd, spp, n, n + 1) for n in range(spp)])
    torch.cuda.synchronize()
    new.close()
    old.close()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.any(a.reshape(-1, 4)[:, :3] != 0.0) and np.all(a[:, 3::4] == 1.0)
    assert np.array_equal(a, b), "%d values differ" % int((a != b).sum())


@pytest.mark.parametrize("ap", [0.0, 0.15])
def test_lockstep_statistical_mode(ap):
    """The statistical RNG composes with force_flags (the forced scene launches <68> / <76>): its
    stream is seeded per path, so the draws dropped at a path's end are unobservable."""
    w, h, spp = 40, 24, 64
    a, b = _frames(w, h, spp, 77, ap, api.RNG_XOSHIRO)
    _check(a, b, w, h, spp)
