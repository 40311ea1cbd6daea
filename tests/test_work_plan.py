"""The work plan of a render (csrc/ptmi_plan.h plan_work) through ptmi_diag_work_plan_host: no scene, no device.

Golden plans: tests/golden/work_plans.json holds requests and the plans that the planning code inside
render_frame computed for them before it became plan_work (commit 25272fc; recorded by a throw-away program
holding those lines verbatim) -- automatic and explicit chunk counts, sample shares, raster and diagonal tile
splits at every offset, ranks that own nothing, the knobs, a caller's list, the 2^25 / 2^26 path-pool limits, and
the study build's split form.  A refactor of the plan must reproduce every one of them.

Invariants: what every plan must satisfy, over the table and over random requests from a fixed seed.
"""
import json
import os
import random

import pytest

from ptmi import api

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "work_plans.json")
F_GROUPS, F_TLIST = 1, 128
Q = {k: i for i, k in enumerate(api.PLAN_REQUEST_FIELDS)}


ECHO = ("s_begin", "s_end", "tile_stride", "tile_offset")  # the request's own values: checked as an invariant
GOLDEN_FIELDS = tuple(k for k in api.PLAN_FIELDS if k not in ECHO)
KNOBS = api.PLAN_REQUEST_FIELDS[14:]


def _table():
    """The table's cases as {"q": the 21 request words, "p": [status, plan...], "t": first owned tiles}: a case
    lists the knobs only where they differ from the defaults a scene of its flags has."""
    doc = json.load(open(GOLDEN))
    assert tuple(doc["request_fields"]) + KNOBS == api.PLAN_REQUEST_FIELDS
    assert tuple(doc["plan_fields"][1:]) == GOLDEN_FIELDS and tuple(doc["knob_defaults"]) == KNOBS
    cases = []
    for c in doc["cases"]:
        knobs = dict(doc["knob_defaults"], min_chunk=64 if c[0][10] & F_GROUPS else 32)
        knobs.update(c[3] if len(c) > 3 else {})
        cases.append({"q": c[0] + [knobs[k] for k in KNOBS], "p": c[1], "t": c[2] if len(c) > 2 else []})
    return cases


TABLE = _table()


def _plan(q, n_tiles=0):
    """(status, plan dict or None, tiles)"""
    try:
        p, t = api.work_plan_host(q, n_tiles)
    except api.PtmiError as e:
        return e.code, None, []
    return 0, p, [int(v) for v in t]


def test_golden_plans():
    assert len(TABLE) >= 675
    bad = []
    for c in TABLE:
        status, p, tiles = _plan(c["q"], len(c["t"]))
        got = [status] + ([p[k] for k in GOLDEN_FIELDS] if p else [])
        if got != c["p"] or tiles != c["t"]:
            bad.append((c["q"], c["p"], got, c["t"], tiles))
    assert not bad, "%d of %d plans differ; first: request %s expected %s got %s (tiles %s / %s)" % (
        (len(bad), len(TABLE)) + bad[0])


def test_the_table_holds_the_cases_it_is_meant_to():
    """(so that an edit of the table cannot quietly drop a kind of case)"""
    qs = [c["q"] for c in TABLE]
    ok = [c for c in TABLE if c["p"][0] == 0]
    assert {q[Q["flags"]] for q in qs} >= {0, 1, 5, 65, 31, 271}
    assert {q[Q["resident_waves"]] for q in qs} >= {4096, 16, 0}
    assert {(q[Q["width"]], q[Q["height"]]) for q in qs} >= {(64, 48), (100, 75), (1280, 960)}
    for w, stride in ((64, 1), (64, 2), (64, 8), (64, 3), (64, 50), (100, 13), (1280, 2), (1280, 8)):
        assert {q[Q["tile_offset"]] for q in qs if q[Q["width"]] == w and q[Q["tile_stride"]] == stride} >= set(
            range(stride)), (w, stride)
    assert any(c["p"][7] == 0 for c in ok)  # a rank that owns nothing
    assert any(c["p"][9] == 1 for c in ok) and any(c["q"][Q["tile_stride"]] > 1 and c["p"][9] == 0 for c in ok)
    assert {q[Q["chunks"]] for q in qs} >= {0, 1, 2, 5000}
    assert {q[Q["sample_end"]] - q[Q["sample_begin"]] for q in qs} >= {0, 1, 512, 513, 2048}
    assert {q[Q["n_list"]] for q in qs if q[Q["has_list"]]} >= {1, 7}
    assert any(q[Q["tail_tiles"]] == 5 for q in qs) and any(q[Q["min_chunk"]] == 128 for q in qs)
    assert {q[Q["tail_split"]] for q in qs} >= {1, 2, 4}
    # the 2^25 bound forces two chunks on a tile-list launch of 2^26 samples; the 2^26 moment limit is an error
    assert any(c["q"][Q["samples"]] == 1 << 26 and c["p"][8] & F_TLIST and c["q"][Q["chunks"]] <= 1 and c["p"][3] == 2
               for c in ok)
    assert any(c["p"] == [-1] and c["q"][Q["samples"]] == 1 << 26 and c["q"][Q["moments"]] for c in TABLE)
    assert any(c["p"] == [-4] for c in TABLE) and any(c["p"][11] == 1 for c in ok)  # the split form


def _check_invariants(q, p):
    rng = q[Q["sample_end"]] - q[Q["sample_begin"]]
    assert p["n_whole"] + p["n_tail"] == p["owned_tiles"], (q, p)
    total = p["n_long"] * p["chunk_len"] + (p["nchunks"] - p["n_long"]) * p["tail_len"]
    assert p["nchunks"] >= 1 and p["n_long"] <= p["nchunks"] and p["chunk_len"] >= 1 and p["tail_len"] >= 1, (q, p)
    assert total >= rng, (q, p)
    if rng == 0:
        # the plan's `range == 0` rule: one chunk of length 1 that the kernels clip to nothing, every tile whole
        # (in the split form, which keeps every tile chunked, an empty range is never planned: split is 0)
        assert (p["nchunks"], p["chunk_len"], p["n_tail"], p["split"]) == (1, 1, 0, 0), (q, p)
    else:  # no chunk is empty: without the last one the rest do not cover the range
        last = p["tail_len"] if p["nchunks"] > p["n_long"] else p["chunk_len"]
        assert total - last < rng, (q, p)
    automatic_mesh = q[Q["chunks"]] == 0 and (q[Q["flags"]] & F_GROUPS) and not p["split"]
    if not automatic_mesh:
        assert p["n_long"] == p["nchunks"] and p["tail_len"] == p["chunk_len"], (q, p)
    if p["launch_flags"] & F_TLIST:
        assert max(p["chunk_len"], p["tail_len"]) <= 1 << 25, (q, p)
    assert (p["s_begin"], p["s_end"], p["tile_stride"], p["tile_offset"]) == tuple(
        q[Q[k]] for k in ("sample_begin", "sample_end", "tile_stride", "tile_offset")), (q, p)


def test_invariants_of_the_table():
    n = 0
    for c in TABLE:
        status, p, _ = _plan(c["q"])
        if status == 0:
            _check_invariants(c["q"], p)
            n += 1
    assert n >= 660


def _random_request(r):
    w, h = r.choice(((8, 8), (64, 48), (100, 75), (37, 91), (640, 8), (1280, 960)))
    samples = r.choice((1, 2, 63, 64, 65, 1000, 2048, 100000, 1 << 26, (1 << 27) + 5))
    b = r.randrange(0, samples + 1)
    e = r.choice((b, samples, r.randrange(b, samples + 1), min(samples, b + 1)))
    stride = r.choice((1, 1, 2, 3, 4, 5, 8, 13, 16, 1000, 30000))
    flags = r.choice((0, 1, 5, 65, 31, 63, 271, 335, 8, 15))
    has_list = r.random() < 0.15
    if has_list:
        stride = 1
    return [w, h, samples, b, e, stride, r.randrange(stride), r.choice((0, 0, 0, 1, 2, 3, 7, 100, 1 << 20)),
            int(has_list), r.choice((1, 7, 100)) if has_list else 0, flags, r.choice((0, 1, 16, 1024, 4096, 8192)),
            int(has_list or r.random() < 0.3), r.choice((0, 0, 0, 0, 1, 64, 500)),
            r.choice((0, 0, 5, 4096)), r.choice((1, 6, 50)), r.choice((1, 32, 50)), r.choice((1, 48, 64)),
            r.choice((1, 2, 32, 64, 128)), r.choice((1, 2, 4, 9)), r.choice((0, 0, 1, 8, 16, 100))]


def test_invariants_of_random_requests():
    r = random.Random(20251021)
    planned = 0
    for _ in range(600):
        q = _random_request(r)
        status, p, _ = _plan(q)
        assert status in (0, -1, -4), q
        if status == 0:
            _check_invariants(q, p)
            planned += 1
    assert planned > 400


@pytest.mark.parametrize("flags", [0, 1], ids=["raster", "diagonal"])
@pytest.mark.parametrize("w,h,stride", [(64, 48, 1), (64, 48, 2), (64, 48, 8), (64, 48, 3), (64, 48, 50),
                                        (100, 75, 2), (100, 75, 13), (1280, 960, 8)])
def test_ownership_partitions_the_tiles(flags, w, h, stride):
    """Over all offsets of a stride the owned tiles partition [0, tiles); the mesh flags take the diagonal where
    the tile rows divide by the stride, and tile (x, y) then belongs to rank (x + y) mod stride."""
    tiles_x, tiles = (w + 7) // 8, ((w + 7) // 8) * ((h + 7) // 8)
    diagonal = bool(flags & F_GROUPS) and stride > 1 and tiles_x % stride == 0
    seen = []
    for off in range(stride):
        q = [w, h, 64, 0, 64, stride, off, 0, 0, 0, flags, 4096, 0, 0, 0, 6, 32, 48, 64 if flags else 32, 4, 0]
        status, p, t = _plan(q, tiles)
        assert status == 0 and p["tlist"] == int(diagonal) and len(t) == p["owned_tiles"]
        assert bool(p["launch_flags"] & F_TLIST) == diagonal
        for k in t:
            assert (k % tiles_x + k // tiles_x) % stride == off if diagonal else k % stride == off
        seen += t
    assert sorted(seen) == list(range(tiles))


def test_refusals_carry_the_render_messages():
    q = [64, 48, 2048, 9, 8, 2, 1, 0, 0, 0, 0, 4096, 0, 0, 0, 6, 32, 48, 32, 4, 0]
    with pytest.raises(api.PtmiError, match=r"bad render arguments \(samples 2048 range \[9,8\) tiles 1/2\)"):
        api.work_plan_host(q)
    q = [64, 48, 1 << 26, 0, 1 << 26, 1, 0, 1, 0, 0, 1, 4096, 1, 0, 0, 6, 32, 48, 64, 4, 0]
    with pytest.raises(api.PtmiError, match=r"a pooled work item of 67108864 samples \(>= 2\^26\); use more chunks"):
        api.work_plan_host(q)
    with pytest.raises(api.PtmiError):  # a malformed call: too few words
        api.work_plan_host(q[:-1])
    with pytest.raises(api.PtmiError):  # no frame
        api.work_plan_host([0] + q[1:])


def test_a_callers_list_leaves_the_tile_buffer_alone():
    q = [64, 48, 64, 0, 64, 1, 0, 0, 1, 7, 1, 4096, 1, 0, 0, 6, 32, 48, 64, 4, 0]
    p, t = api.work_plan_host(q, 16)
    assert p["owned_tiles"] == 7 and p["launch_flags"] & F_TLIST and p["tlist"] == 0 and len(t) == 0
