"""CPU: the inputs and restatements of tests/_unique_ref.py against independent references —
every expected-by-construction list against ``np.unique`` of its keys, ``trunc_long`` against
``Tensor.long()`` where that cast is defined, ``remap_ref`` / ``coalesce_ref`` against the
oracle's dict loop and scipy — and the comparison helper against the three wrong lists a slipped
guard in csrc/unique.hip would produce (an element dropped, duplicated, a pair swapped)."""
import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests import _unique_ref as U

GEOMETRY = U.geometry_cases()
FAR = U.far_cases()
FLOATS = U.float_cases()


def _check_pair(keys, expected):
    assert keys.dtype == np.int64 and expected.dtype == np.int64
    assert np.array_equal(expected, np.unique(keys))
    got = torch.from_numpy(expected.copy())
    assert U.same_list(got, expected)
    if expected.size >= 2:
        for what, wrong in U.perturbed(expected).items():
            assert not U.same_list(torch.from_numpy(wrong), expected), what
    assert not U.same_list(got.to(torch.int32), expected)


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_geometry_cases_are_their_np_unique(name):
    """bits_at on every word / thread / tile / LDS boundary case of the GPU file."""
    keys, expected, guard = GEOMETRY[name]()
    assert guard
    _check_pair(keys, expected)


@pytest.mark.parametrize("name", list(FAR))
def test_far_cases_are_their_np_unique(name):
    """with_far / far_keys on every window-edge and far-list case of the GPU file."""
    keys, expected, guard = FAR[name]()
    assert guard
    _check_pair(keys, expected)


def test_far_cases_sit_where_they_claim():
    """The far list (keys at or past lo + 2^24) of the farK cases has K distinct keys; the
    single-copy lists are exactly K long; the 1-to-3-copy lists have one run of equal keys over
    sorted positions 1,023/1,024 and one over 4,095/4,096 when they are long enough."""
    for k in U.FAR_COUNTS:
        for kind in ("single", "copies"):
            keys, expected, _ = FAR[f"far{k}-{kind}"]()
            far = np.sort(keys[keys >= keys.min() + U.CAP_BITS])
            assert len(np.unique(far)) == k
            if kind == "single":
                assert len(far) == k
            else:
                for edge in (U.FAR_THREADS, U.FAR_LDS):
                    if len(far) > edge:
                        assert far[edge - 1] == far[edge], (k, edge)
    keys, _, _ = FAR["far-int64-max-workspace"]()
    assert (keys >= U.CAP_BITS).sum() == U.FAR_LDS + 1 and keys.max() == U.INT64_MAX


def test_geometry_cases_sit_where_they_claim():
    """wordsW: the span is exactly W words of range_words; mid-empty: no key in tile 1
    (kTileWords · 32 bits) and one at the first bit of tile 2; window-sparse: span kCapBits - 1
    and a key in each of the kMaxTiles tiles."""
    for lo in U.LOS:
        tag = "lo%d" % (0 if lo < 0 else 40)
        for words in (1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097):
            _, e, _ = GEOMETRY[f"words{words}-{tag}"]()
            assert e[0] == lo and (e[-1] - lo + 1 + 31) // 32 == words
            assert e[-1] - lo == words * 32 - 1
        _, e, _ = GEOMETRY[f"words4097-mid-empty-{tag}"]()
        assert not ((e - lo >= U.TILE_BITS) & (e - lo < 2 * U.TILE_BITS)).any()
        assert (e - lo == 2 * U.TILE_BITS).any()
        _, e, _ = GEOMETRY[f"window-sparse-{tag}"]()
        assert e[-1] - e[0] == U.CAP_BITS - 1
        assert len(np.unique((e - lo) // U.TILE_BITS)) == U.MAX_TILES


@pytest.mark.parametrize("n", [n for n in U.SIZES])
def test_sized_inputs(n):
    """sized_input: exactly n keys (the kGrid · 256 and kGrid · 4,096 grid caps), the minimum
    last and the maximum before it, the expected list by construction."""
    for lo in U.LOS:
        keys, expected = U.sized_input(n, lo)
        assert len(keys) == n
        assert keys[-1] == keys.min() == lo
        if n > 1:
            assert keys[-2] == keys.max()
        _check_pair(keys, expected)


def test_dense_and_with_far_small():
    """dense, with_far, far_keys and bits_at with per-position repeats at sizes a host sort
    handles, at both window starts and at lo = INT64_MIN; the first far key is lo + kCapBits."""
    for lo in U.LOS + (U.INT64_MIN,):
        for stride in (1, 3):
            keys, expected = U.dense(lo, 1000, stride)
            _check_pair(keys, expected)
            keys, expected = U.with_far((keys, expected), U.far_keys(lo, 7, (3, 1, 2)))
            _check_pair(keys, expected)
    keys, expected = U.bits_at(5, [9, 0, 9, 2], [1, 2, 3])
    assert sorted(keys.tolist()) == [5, 7, 7, 14, 14, 14] and expected.tolist() == [5, 7, 14]


def test_trunc_long_is_tensor_long_where_defined():
    """trunc_long against Tensor.long() on finite in-range values (±0.999…, -0.0, denormals,
    ±(2^63 - 2^39), halves), and TruncSrc's rule ``!(fabsf(x) < 2^63)`` → INT64_MIN stated for
    NaN, ±inf, ±2^63 and beyond."""
    below1 = np.nextafter(np.float32(1), np.float32(0))
    x = np.array([0.999, -0.999, below1, -below1, -0.0, 0.0, 1.0, -1.0, 1.5, -1.5, 2.5, -2.5,
                  16777215.0, 16777216.0, -16777216.0, 3e9, -3e9, U.F63, -U.F63,
                  1e-45, -1e-45, 1e-42, -1e-42, 1.1754942e-38, 8388607.5, -8388607.5],
                 dtype=np.float32)
    rng = np.random.default_rng(0)
    x = np.concatenate([x, (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 18, 4000))
                        .astype(np.float32)])
    got = U.trunc_long(x)
    assert got.dtype == np.int64
    assert np.array_equal(got, torch.tensor(x).long().numpy())
    assert got[:6].tolist() == [0] * 6 and got[17:19].tolist() == [2 ** 63 - 2 ** 39,
                                                                 -(2 ** 63 - 2 ** 39)]
    # -2^63 is representable and in range for a C++ cast, but TruncSrc's |x| < 2^63 sends it to
    # INT64_MIN as well — the same value
    nan, inf = float("nan"), float("inf")
    out = np.array([nan, inf, -inf, 2.0 ** 63, -2.0 ** 63, -2.0 ** 63 - 2.0 ** 40, 1e30, -1e30,
                    3.4e38], dtype=np.float32)
    assert (U.trunc_long(out) == U.INT64_MIN).all()


@pytest.mark.parametrize("name", list(FLOATS))
def test_float_cases(name):
    """Every float case of the GPU file: trunc_long equals Tensor.long() on its in-range values
    and INT64_MIN elsewhere; lds-switch spans the kLdsWords boundary from lo = -3."""
    x, guard = FLOATS[name]
    assert guard and x.dtype == np.float32
    keys = U.trunc_long(x)
    _check_pair(keys, U.unique_ref(keys))
    fin = np.isfinite(x) & (np.abs(x) < np.float32(2.0 ** 63))
    assert np.array_equal(keys[fin], torch.tensor(x[fin]).long().numpy())
    assert (keys[~fin] == U.INT64_MIN).all()
    if name == "lds-switch":
        assert len(np.unique(keys)) == 7 and keys.min() == -3


def test_remap_ref_is_the_oracle_dict_loop():
    """remap_ref against the oracle's remap_ids (Interaction.__generate_set) on every remap
    case up to 5,000 keys and a random one."""
    cases = dict(U.remap_cases())
    rng = np.random.default_rng(4)
    cases["random"] = rng.integers(-50, 50, size=700)
    for name, keys in cases.items():
        if len(keys) > 5000:
            continue
        ids, uniq = U.remap_ref(keys)
        user, _ = O.remap_ids(zip(keys.tolist(), keys.tolist()))
        assert uniq.tolist() == list(user.keys()), name
        assert ids.tolist() == [user[k] for k in keys.tolist()], name
        assert ids.dtype == np.int32 and uniq.dtype == np.int64


def test_remap_cases_have_their_distinct_counts():
    """The remap cases hold what bits_for(2 * n) needs: n, 1, n - 1 and 1 + n/2 distinct keys
    (n_seg of k_pad_segments); descending first appearances; a key at both ends."""
    cases = U.remap_cases()
    for n in (1, 2, 255, 256, 257, 1024, 1 << 16, (1 << 16) + 1):
        assert len(np.unique(cases[f"n{n}-distinct"])) == n == len(cases[f"n{n}-distinct"])
        assert len(np.unique(cases[f"n{n}-equal"])) == 1
        if n > 2:
            assert len(np.unique(cases[f"n{n}-n-1"])) == n - 1
            assert len(np.unique(cases[f"n{n}-half+1"])) == 1 + n // 2
    d = cases["descending"]
    first = d[np.sort(np.unique(d, return_index=True)[1])]
    assert (np.diff(first) < 0).all()
    e = cases["first-and-last"]
    assert e[0] == e[-1] and (e[1:-1] != e[0]).all()


def test_coalesce_ref_is_scipy_csr():
    """coalesce_ref against scipy's canonical csr_matrix with summed float32 ones, the top
    corner (n_rows - 1, n_cols - 1) — the largest key of bits_for(n_rows * n_cols) — present;
    and the float32 arithmetic behind the 2^24 + 1 multiplicity case."""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    shapes = [(3, 85), (257, 1), (1, 300), (16, 16), (40, 7)]
    for k, (R, C) in enumerate(shapes):
        for n in (1, 5, 257, 2000):
            rows, cols = U.corner_coo(n, R, C, seed=10 * k + n)
            rowptr, col, val = U.coalesce_ref(rows, cols, R, C)
            m = sp.csr_matrix((np.ones(n, np.float32), (rows, cols)), shape=(R, C),
                              dtype=np.float32)
            m.sum_duplicates()
            m.sort_indices()
            assert np.array_equal(rowptr, m.indptr) and np.array_equal(col, m.indices)
            assert np.array_equal(val.view(np.uint32), m.data.view(np.uint32))
            assert (rows == R - 1).any() and (cols[rows == R - 1] == C - 1).any()
    del rng
    # 2^24 + 1 ones summed in float32 stay at 2^24, which is also the float32 of the count
    assert np.float32(2 ** 24 + 1) == np.float32(16777216.0)
    assert np.float32(16777216.0) + np.float32(1.0) == np.float32(16777216.0)


def test_normalize_ref_order_and_dtype():
    """normalize_ref is float32 (d_r · v) · d_c in that order (k_normalize_values), d_r · v
    without a column scale, on a hand-written CSR with an empty row."""
    rowptr = np.array([0, 2, 2, 5])
    col = np.array([0, 2, 0, 1, 2])
    val = np.array([1, 3, 2, 1, 7], np.float32)
    d = np.array([0.1, 0.0, 0.3], np.float32)
    out = U.normalize_ref(rowptr, col, val, d, d)
    want = [(d[r] * v) * d[c] for r, c, v in zip([0, 0, 2, 2, 2], col, val)]
    assert out.dtype == np.float32
    assert np.array_equal(out.view(np.uint32), np.array(want, np.float32).view(np.uint32))
    out = U.normalize_ref(rowptr, col, val, d, None)
    assert np.array_equal(out, np.array([d[0] * 1, d[0] * 3, d[2] * 2, d[2] * 1, d[2] * 7],
                                        np.float32))
