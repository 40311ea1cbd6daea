"""ptmi_select_tiles (the order-preserving compaction of the tiles still above the threshold) and
ptmi_finalize_counts against their numpy statements in ptmi/error.py: exact equality, since the
kernels only compare, count and copy (select) or multiply once (finalize).

Sizes sit around the kernel's block edges -- a wave holds 64 candidates, the workgroup walks 1024 per
step -- and at the product's frame (1280x960: 19,200 tiles)."""
import ctypes

import numpy as np
import pytest

from ptmi import api, error

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 19200)
N_ERR = 19200
THRESHOLD = 0.5


@pytest.fixture(scope="module")
def tile_err():
    """Random errors with planted ties, NaN and +/-inf, some of them at block edges."""
    rng = np.random.RandomState(11)
    e = rng.rand(N_ERR)
    e[rng.choice(N_ERR, 900, replace=False)] = THRESHOLD  # ties: dropped
    e[rng.choice(N_ERR, 900, replace=False)] = np.nan     # dropped
    e[rng.choice(N_ERR, 900, replace=False)] = np.inf     # kept
    e[rng.choice(N_ERR, 300, replace=False)] = -np.inf
    e[[0, 63, 64, 1023, 1024]] = [0.9, np.nan, 0.9, THRESHOLD, np.inf]
    return e


def _select(torch, err_dev, in_tiles, n_in):
    out = torch.full((max(n_in, 1) + 8,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    lst = None if in_tiles is None else torch.tensor(in_tiles.view(np.int32), dtype=torch.int32, device="cuda")
    api.select_tiles(err_dev.data_ptr(), 0 if lst is None or n_in == 0 else lst.data_ptr(), n_in, THRESHOLD,
                     out.data_ptr(), count.data_ptr())
    torch.cuda.synchronize()
    n = int(count.item())
    out = out.cpu().numpy()
    assert np.all(out[n:] == -7), "wrote past the kept tiles"
    return out[:n].view(np.uint32), n


@pytest.mark.parametrize("n_in", SIZES)
def test_select_all_tiles(tile_err, n_in):
    import torch
    dev = torch.tensor(tile_err, dtype=torch.float64, device="cuda")
    exp, n_exp = error.select_tiles_reference(tile_err, None, n_in, THRESHOLD)
    for _ in range(2):  # determinism
        got, n = _select(torch, dev, None, n_in)
        assert n == n_exp and np.array_equal(got, exp)
    assert n_in < 64 or 0 < n_exp < n_in


@pytest.mark.parametrize("n_in", SIZES)
def test_select_from_a_shuffled_list(tile_err, n_in):
    import torch
    dev = torch.tensor(tile_err, dtype=torch.float64, device="cuda")
    lst = np.random.RandomState(n_in + 1).permutation(N_ERR)[:n_in].astype(np.uint32)
    exp, n_exp = error.select_tiles_reference(tile_err, lst, n_in, THRESHOLD)
    for _ in range(2):
        got, n = _select(torch, dev, lst, n_in)
        assert n == n_exp and np.array_equal(got, exp)


def test_select_refuses_aliased_lists(tile_err):
    import torch
    dev = torch.tensor(tile_err, dtype=torch.float64, device="cuda")
    lst = torch.arange(64, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(api.PtmiError) as e:
        api.select_tiles(dev.data_ptr(), lst.data_ptr(), 64, THRESHOLD, lst.data_ptr(), count.data_ptr())
    assert e.value.code == api.PTMI_ERR_ARG


def test_finalize_counts():
    import torch
    rng = np.random.RandomState(12)
    npix = 1000  # (not a multiple of the workgroup)
    sums = rng.rand(npix, 4) * 40
    sums[:, 3] = rng.choice([0.0, 16.0, 48.0], npix)
    sums[sums[:, 3] == 0, :3] = 0.0
    sums[5, :3] = 3.0  # stray sums under a zero count still give RGB 0
    sums[5, 3] = 0.0
    dev = torch.tensor(sums.reshape(-1), dtype=torch.float64, device="cuda")
    out = torch.full((npix * 4,), -1.0, dtype=torch.float64, device="cuda")
    api.finalize_counts(dev.data_ptr(), out.data_ptr(), npix)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, error.finalize_counts_reference(sums.reshape(-1)))
    assert not got.reshape(-1, 4)[5, :3].any() and {0.0, 16.0, 48.0} == set(sums[:, 3])
    # a uniform count: ptmi_finalize's output bit for bit
    sums[:, 3] = 48.0
    dev = torch.tensor(sums.reshape(-1), dtype=torch.float64, device="cuda")
    out2 = torch.empty(npix * 4, dtype=torch.float64, device="cuda")
    err = ctypes.create_string_buffer(256)
    assert api.load_library().ptmi_finalize(dev.data_ptr(), out2.data_ptr(), npix, 48, None, err, len(err)) == 0
    api.finalize_counts(dev.data_ptr(), out.data_ptr(), npix)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
