"""GPU: hgd_kg_expand (csrc/ingest.hip) called through the C ABI, not through KnowledgeGraph, which
would size its tables by the largest id.

The reference is numpy: the five blocks (h, r+2, t) | (t, r+n0+2, h) | (t, r+n0, h) | (u, 0, i) |
(i, 1, u) with n0 = max(r) + 1 over the accepted triples (0 for none), their int32 copies, and the
four statistics. All integers, all compared exactly; inputs, outputs and stats are carved out of
one guarded device buffer (tests/_arena.py) and the outputs start as FILL.

First reached here in k_kg_stats: several live waves and several workgroups feeding the wave
reductions and the atomics (every shape from 64 up); ``widest`` taking n_cf (n_cf > n); the
grid-stride loops past the 1024-block cap, in the triple loop and in the record loop (2^18 + 69
entries); ids at the two limits themselves; rejected entries counted across waves and blocks and
kept out of the maxima.
"""
import numpy as np
import pytest

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from tests._arena import Arena

pytestmark = pytest.mark.gpu

ID_LIMIT = 0x7FFFFFFE   # kKgIdLimit: ids below it are accepted
REL_LIMIT = 0x3FFFFFFF  # kKgRelLimit
FILL = -7
BIG = 262_144 + 69      # 1024 blocks x 256 threads, one more wave and a tail of 5
SHAPES = [(1, 0), (0, 1), (63, 0), (64, 65), (257, 3), (3, 1000), (BIG, 5), (5, BIG)]
I64 = np.int64


def _data(n, n_cf, seed=0):
    rng = np.random.default_rng(seed + 31 * n + n_cf)
    h, t = rng.integers(0, 1000, n, dtype=I64), rng.integers(0, 1000, n, dtype=I64)
    r = rng.integers(0, 20, n, dtype=I64)
    u, i = rng.integers(0, 3000, n_cf, dtype=I64), rng.integers(0, 3000, n_cf, dtype=I64)
    return h, r, t, u, i


def _reference(h, r, t, u, i):
    n, n_cf = len(h), len(u)
    ok = (h >= 0) & (h < ID_LIMIT) & (t >= 0) & (t < ID_LIMIT) & (r >= 0) & (r < REL_LIMIT)
    ok_cf = (u >= 0) & (u < ID_LIMIT) & (i >= 0) & (i < ID_LIMIT)
    ent = int(max(h[ok].max(), t[ok].max())) + 1 if ok.any() else 0
    every = max(ent, int(max(u[ok_cf].max(), i[ok_cf].max())) + 1 if ok_cf.any() else 0)
    n0 = int(r[ok].max()) + 1 if ok.any() else 0
    stats = [ent, every, n0, int((~ok).sum() + (~ok_cf).sum())]
    zeros, ones = np.zeros(n_cf, I64), np.ones(n_cf, I64)
    H = np.concatenate([h, t, t, u, i])
    R = np.concatenate([r + 2, r + n0 + 2, r + n0, zeros, ones])
    T = np.concatenate([t, h, h, i, u])
    assert len(H) == len(R) == len(T) == 3 * n + 2 * n_cf
    return H, R, T, stats


def _expand(dev, h, r, t, u, i):
    """Runs the entry on guarded copies; returns (h_out, r_out, t_out, h32, r32, t32, stats)."""
    n, n_cf = len(h), len(u)
    total = 3 * n + 2 * n_cf
    ar = Arena()
    for name, x in (("h", h), ("r", r), ("t", t), ("u", u), ("i", i)):
        assert x.dtype == np.int64
        ar.add(name, x)
    for name in ("h_out", "r_out", "t_out"):
        ar.add(name, np.full(total, FILL, I64), out=True)
    for name in ("h32", "r32", "t32"):
        ar.add(name, np.full(total, FILL, np.int32), out=True)
    ar.add("stats", np.full(4, FILL, I64), out=True)
    ar.upload(dev)
    kg = [ar.ptr(x) if n else None for x in "hrt"]
    cf = [ar.ptr(x) if n_cf else None for x in "ui"]
    outs = [ar.ptr(x) if total else None for x in ("h_out", "r_out", "t_out", "h32", "r32", "t32")]
    nat.check(nat.load().hgd_kg_expand(*kg, n, *cf, n_cf, *outs, ar.ptr("stats"),
                                       nat.stream_handle(dev)), "hgd_kg_expand")
    got = ar.check((n, n_cf))
    return [got[x] for x in ("h_out", "r_out", "t_out", "h32", "r32", "t32", "stats")]


def _check(dev, h, r, t, u, i, what):
    H, R, T, stats = _reference(h, r, t, u, i)
    h_out, r_out, t_out, h32, r32, t32, got = _expand(dev, h, r, t, u, i)
    assert got.tolist() == stats, (what, got.tolist(), stats)
    for name, a, b in (("h", h_out, H), ("r", r_out, R), ("t", t_out, T)):
        assert a.dtype == np.int64 and np.array_equal(a, b), (what, name)
    for name, a, b in (("h32", h32, H), ("r32", r32, R), ("t32", t32, T)):
        assert a.dtype == np.int32 and np.array_equal(a, b.astype(np.int32)), (what, name)
    return stats


# ---- shapes, with the maxima in the last element and in element 0 ------------------------------
@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("n,n_cf", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_shapes_with_the_maxima_at_an_end(dev, n, n_cf, where):
    """The largest entity id, CF id and relation sit in one element only: the last (the tail
    thread of the last live wave, or of the grid-stride loop's second trip) or element 0. A
    reduction that drops a wave, a block or a tail loses one of the three counts."""
    h, r, t, u, i = _data(n, n_cf)
    at = -1 if where == "last" else 0
    if n:
        (t if where == "last" else h)[at] = 5000
        r[at] = 40
    if n_cf:
        (i if where == "last" else u)[at] = 9000
    stats = _check(dev, h, r, t, u, i, (n, n_cf, where))
    assert stats == [5001 if n else 0, 9001 if n_cf else 5001, 41 if n else 0, 0]


def test_entity_maximum_above_every_cf_id(dev):
    """stats[1] carries the entity maximum over when no CF id exceeds it (``all = ent``)."""
    h, r, t, u, i = _data(300, 700)
    h[299] = 70_000
    assert _check(dev, h, r, t, u, i, "entity above CF")[:2] == [70_001, 70_001]


def test_empty_call_with_null_inputs(dev):
    e = np.zeros(0, I64)
    got = _expand(dev, e, e, e, e, e)
    assert got[6].tolist() == [0, 0, 0, 0]


# ---- the id limits ------------------------------------------------------------------------------
def test_largest_accepted_ids(dev):
    """Entity id 0x7ffffffd in h, in t, as a user and as an item, and relation 0x3ffffffe: all
    accepted, and r + n0 + 2 = 0x7fffffff still fits the int32 copy."""
    for col in range(4):
        h, r, t, u, i = _data(70, 70, seed=col)
        (h, t, u, i)[col][33] = ID_LIMIT - 1
        stats = _check(dev, h, r, t, u, i, ("largest id", col))
        assert stats[3] == 0 and stats[1] == ID_LIMIT
        assert stats[0] == ID_LIMIT if col < 2 else stats[0] <= 1000
    h, r, t, u, i = _data(70, 70)
    r[69] = REL_LIMIT - 1
    assert _check(dev, h, r, t, u, i, "largest relation")[2:] == [REL_LIMIT, 0]


BAD_ONE = [("h", ID_LIMIT), ("t", ID_LIMIT), ("u", ID_LIMIT), ("i", ID_LIMIT), ("r", REL_LIMIT),
           ("h", -1), ("r", -1), ("t", -1), ("u", -1), ("i", -1), ("h", 2 ** 31), ("i", 2 ** 40),
           ("r", 2 ** 31 - 1), ("t", -(2 ** 63))]


@pytest.mark.parametrize("col,value", BAD_ONE, ids=[f"{c}={v:#x}" for c, v in BAD_ONE])
def test_one_bad_entry(dev, col, value):
    """The first id past each limit, a negative id in each of the five inputs and ids beyond
    int32: one rejected entry each, and the counts are those of the other entries."""
    h, r, t, u, i = _data(70, 70)
    dict(h=h, r=r, t=t, u=u, i=i)[col][66] = value
    stats = _check(dev, h, r, t, u, i, (col, value))
    assert stats[3] == 1 and stats[0] <= 1000 and stats[1] <= 3000 and stats[2] <= 20


@pytest.mark.parametrize("n,n_cf", [(700, 900), (BIG, 5), (5, BIG)],
                         ids=["3-4 blocks", "strided triples", "strided records"])
def test_bad_entries_across_waves_and_blocks(dev, n, n_cf):
    """k rejected entries spread over the inputs (every 97th triple and every 89th record, the
    first and the last of each included): stats[3] == k exactly. Each rejected entry also holds
    an id or a relation above every accepted one, which must not reach the maxima."""
    h, r, t, u, i = _data(n, n_cf)
    kg_at = sorted(set(range(0, n, 97)) | {n - 1})
    cf_at = sorted(set(range(0, n_cf, 89)) | {n_cf - 1})
    for k, e in enumerate(kg_at):
        if k % 3 == 0:
            h[e], r[e] = 50_000, -1          # a large head in a triple with a bad relation
        elif k % 3 == 1:
            t[e], r[e] = ID_LIMIT, 500       # a large relation in a triple with a bad tail
        else:
            h[e], t[e], r[e] = -5, 60_000, REL_LIMIT   # two faults: still one entry
    for k, e in enumerate(cf_at):
        if k % 2 == 0:
            u[e], i[e] = 80_000, -1
        else:
            u[e], i[e] = ID_LIMIT + k, 90_000
    stats = _check(dev, h, r, t, u, i, (n, n_cf))
    assert stats[3] == len(kg_at) + len(cf_at)
    assert stats[0] <= 1000 and stats[1] <= 3000 and stats[2] <= 20


def test_rejected_calls(dev):
    lib, st = nat.load(), nat.stream_handle(dev)
    h, r, t, u, i = _data(8, 8)
    ar = Arena()
    for name, x in (("h", h), ("r", r), ("t", t), ("u", u), ("i", i)):
        ar.add(name, x)
    for name in ("a", "b", "c"):
        ar.add(name, np.full(40, FILL, I64), out=True)
        ar.add(name + "32", np.full(40, FILL, np.int32), out=True)
    ar.add("stats", np.full(4, FILL, I64), out=True).upload(dev)
    good = dict(h=ar.ptr("h"), r=ar.ptr("r"), t=ar.ptr("t"), n=8, u=ar.ptr("u"), i=ar.ptr("i"),
                n_cf=8, a=ar.ptr("a"), b=ar.ptr("b"), c=ar.ptr("c"), a32=ar.ptr("a32"),
                b32=ar.ptr("b32"), c32=ar.ptr("c32"), stats=ar.ptr("stats"))
    cases = [dict(n=-1), dict(n_cf=-1), dict(n=0x7FFFFFFF // 3), dict(n_cf=0x7FFFFFFF // 4),
             dict(stats=None), dict(h=None), dict(r=None), dict(t=None), dict(u=None), dict(i=None)]
    for over in cases:
        assert lib.hgd_kg_expand(*dict(good, **over).values(), st) != 0, over
        assert lib.hgd_get_last_error_string().decode().startswith("hgd_kg_expand: ")
    got = ar.check("rejected calls")
    assert all((got[name] == FILL).all() for name in got)
