"""CPU checks of tests/_topk_ref.py: the closed form the GPU edge tests compare with equals the
literal find_k_largest on the builders' short rows (±inf, ±0.0, denormals, k == n_cols), ``plan``
agrees with a brute-force sort, and every builder meets the (in_bin, need, path) it states."""
import numpy as np
import pytest

from oracle import hgd_oracle as O
from tests import _topk_ref as T

N_SMALL = (1, 2, 3, 5, 7, 9, 13, 257, 259)
K_ALL = (1, 2, 3, 5, 7, 129, 255, 256)


def _same(row, k):
    ids, sc = O.topk_closed_form(k, row)
    lit_ids, lit_sc = O.find_k_largest(k, row)
    assert ids == lit_ids, (len(row), k, ids[:8], lit_ids[:8])
    assert T.bits(np.asarray(sc, np.float32)).tolist() == \
        T.bits(np.asarray(lit_sc, np.float32)).tolist()


def test_float_key_orders_like_the_floats():
    inf = np.float32(np.inf)
    tiny = np.array([1, 5, (1 << 23) - 1], np.uint32).view(np.float32)  # denormals
    x = np.concatenate([[-inf, -3e38, -1.0], -tiny[::-1], [-0.0, 0.0], tiny, [1.0, 1.125, 3e38,
                                                                                inf]])
    x = x.astype(np.float32)
    key = T.float_key(x).astype(np.int64)
    zero = int(np.flatnonzero(T.bits(x) == 0x80000000)[0])
    assert key[zero] == key[zero + 1] == 0x80000000  # -0.0 folded onto +0.0
    d = np.diff(key)
    assert (np.delete(d, zero) > 0).all() and d[zero] == 0
    assert T.key_bin(np.float32(1.0)) == T.key_bin(np.float32(1.2499999)) == 0xBF800000 >> 21
    assert T.key_bin(np.float32(1.25)) == T.key_bin(np.float32(1.0)) + 1
    assert T.key_bin(np.float32(0.99999994)) == T.key_bin(np.float32(1.0)) - 1
    assert T.key_bin(T.TIE) == T.key_bin(T.BIN_LO)
    assert T.key_bin(-inf) == 3 and T.key_bin(inf) == 2044 and T.key_bin(T.MASK_VALUE) == 0x319194D7 >> 21


@pytest.mark.parametrize("n", N_SMALL)
def test_closed_form_equals_find_k_largest(n):
    for k in [k for k in K_ALL if k <= n] + [n]:  # k == n_cols included
        for row in T.mixed_rows(n, k, seed=1):
            _same(row, k)
        for kind in T.SPECIAL_KINDS:
            for row in T.special_rows(kind, n, k):
                _same(row, k)


@pytest.mark.parametrize("n_cols,k,in_bin", [(300, 40, 1), (300, 40, 120), (600, 256, 256)])
def test_closed_form_equals_find_k_largest_on_bin_rows(n_cols, k, in_bin):
    for need in T.bin_guard_needs(in_bin, k):
        _same(T.bin_population(n_cols, k, in_bin, need), k)
    ties = np.arange(3, 3 + 2 * in_bin, 2)[: min(in_bin, (n_cols - 3) // 2)]
    _same(T.tie_row(n_cols, min(k, len(ties)), ties, 0), min(k, len(ties)))


@pytest.mark.parametrize("seed", range(6))
def test_plan_agrees_with_a_sort(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 9000))
    row = [rng.standard_normal(n), np.round(rng.standard_normal(n), 1),
           rng.integers(-3, 4, size=n), np.zeros(n)][seed % 4].astype(np.float32)
    for k in sorted({1, min(n, 7), min(n, 256), n}):
        order = np.argsort(-T.float_key(row).astype(np.int64), kind="stable")
        kth_bin = int(T.key_bin(row[order[k - 1:k]])[0])
        bins = T.key_bin(row)
        above = int((bins > kth_bin).sum())
        in_bin = int((bins == kth_bin).sum())
        assert T.plan(row, k) == (kth_bin, k - above, in_bin,
                                  "generic" if in_bin > T.BIN_CAP else "two_pass")
        assert 1 <= k - above <= in_bin


@pytest.mark.parametrize("in_bin", T.BIN_GUARD_IN_BIN)
@pytest.mark.parametrize("k", T.BIN_GUARD_K)
def test_bin_population_meets_its_plan(k, in_bin):
    assert 1 in T.bin_guard_needs(in_bin, k) and min(in_bin, k) in T.bin_guard_needs(in_bin, k)
    for n_cols in T.BIN_GUARD_COLS:
        for need in T.bin_guard_needs(in_bin, k):
            row = T.bin_population(n_cols, k, in_bin, need)
            assert row.dtype == np.float32 and row.shape == (n_cols,)
            inside = (row >= T.BIN_LO) & (row < T.BIN_HI)
            assert int(inside.sum()) == in_bin == len(np.unique(row[inside]))
            assert int((row >= T.BIN_HI).sum()) == k - need
            assert T.plan(row, k)[1:] == (need, in_bin,
                                          "generic" if in_bin > 2048 else "two_pass")
        S = T.bin_guard_rows(n_cols, k, in_bin)
        assert {T.plan(r, k)[1] for r in S} == set(T.bin_guard_needs(in_bin, k))
        assert {T.plan(r, k)[1] for r in S[4:]} == set(T.bin_guard_needs(in_bin, k))
        for r in S[4:]:  # seed window below the bin: the list ends in the bin's need-th key
            last = O.topk_closed_form(k, r)[0][-1]
            assert (r[:k] < T.BIN_LO).all() and T.BIN_LO <= r[last] < T.BIN_HI


@pytest.mark.parametrize("style", T.COMPACTION_STYLES)
@pytest.mark.parametrize("n_cols", T.COMPACTION_N_COLS)
def test_tie_rows_meet_their_plan(n_cols, style):
    for crowded in (True, False):
        cases = T.compaction_rows(n_cols, style, crowded)
        assert 8 <= len(cases) <= 16
        cols = {col for _, col, _ in cases}
        want = {255, 256, 257, 511, 512, n_cols - 1}
        # a style leaves out only the column it cannot hold by definition
        assert cols == want - {"after": {n_cols - 1}, "full_tile": {255}, "late": {255}}[style]
        for k, col, row in cases:
            _, need, in_bin, path = T.plan(row, k)
            ties = np.flatnonzero(row == T.TIE)
            assert ties[need - 1] == col and need + int((row > T.TIE).sum()) == k
            # no seed copy reaches the list: its last entry is the need-th tie
            assert (row[:k] < T.TIE).all() and O.topk_closed_form(k, row)[0][-1] == col
            if crowded:
                assert path == "generic" and in_bin > T.BIN_CAP
            else:
                assert in_bin == len(ties)
            if style == "after":
                assert len(ties) > need  # later ties, to be dropped
            if style == "full_tile":
                t0 = col // T.TILE * T.TILE
                assert (row[t0:t0 + T.TILE] == T.TIE).all()
            if style == "late":
                assert ties[0] >= T.TILE


def test_tie_row_rejects_a_wrong_construction():
    with pytest.raises(AssertionError):
        T.tie_row(600, 10, np.arange(5), 0)        # fewer ties than the need
    with pytest.raises(AssertionError):
        T.bin_population(600, 10, 5, 6)            # need above the bin's population


def test_sweep_cases_reach_every_form():
    """Each loop of for_each_score is taken on both sides of its thresholds (one float4 per
    thread: n_cols // 4 = 256; the first unrolled body: n_cols // 4 = 1024) by some layout."""
    seen = {}
    for n in T.SWEEP_COLS:
        for name in T.SWEEP_LAYOUTS:
            for form in T.sweep_forms(n, *T.layout_geometry(name, n), 12):
                seen.setdefault(form, set()).add(n)
        if n % 4:  # a contiguous tensor alternates aligned and unaligned rows
            assert {"scalar", "tail"} <= T.sweep_forms(n, 0, n, 12)
        assert "scalar" not in T.sweep_forms(n, *T.layout_geometry("ld_mult4", n), 12)
        assert "scalar" in T.sweep_forms(n, *T.layout_geometry("offset1", n), 12)
        assert "scalar" in T.sweep_forms(n, *T.layout_geometry("offset3", n), 12)
    assert seen["scalar"] == set(T.SWEEP_COLS)
    assert seen["tail"] == {n for n in T.SWEEP_COLS if n % 4}
    assert seen["vector"] == set(T.SWEEP_COLS) - {4096, 4097, 4099, 8193}  # n_cols // 4 % 1024 == 0
    assert seen["unrolled"] == {4096, 4097, 4099, 8191, 8193}
