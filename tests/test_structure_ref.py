"""CPU checks of tests/_structure_ref.py on tiny inputs worked out by hand, and of the properties
its generated cases are named for (the GPU edge tests rely on them)."""
import numpy as np
import pytest

from oracle import hgd_oracle as O
from tests import _structure_ref as S

N_LIST = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097)


def test_split_count_and_coo_from_degrees():
    rng = np.random.default_rng(0)
    for total, parts in ((0, 3), (1, 1), (7, 3), (4097, 300)):
        d = S.split_count(rng, total, parts)
        assert d.shape == (parts,) and d.sum() == total and (d >= 0).all()
    rows, cols = S.coo_from_degrees(rng, [2, 0, 1, 3], 3)
    assert rows.tolist() == [0, 0, 2, 3, 3, 3]
    assert cols[3:].tolist() == [0, 1, 2]           # a full row: every column, ascending
    assert cols[0] < cols[1] and 0 <= cols[2] < 3
    rows, cols = S.coo_from_degrees(rng, [0, 0], 5)
    assert rows.size == 0 and cols.size == 0 and cols.dtype == np.int64
    # a skewed draw never picks a column of probability zero
    rows, cols = S.coo_from_degrees(rng, [2, 2], 4, col_p=[0.5, 0.0, 0.5, 0.0])
    assert rows.tolist() == [0, 0, 1, 1] and cols.tolist() == [0, 2, 0, 2]


@pytest.mark.parametrize("n", N_LIST)
def test_graph_exact_has_exactly_n_sorted_unique_entries(n):
    rows, cols, vals, (R, C) = S.graph_exact(n)
    assert len(rows) == len(cols) == len(vals) == n and vals.dtype == np.float32
    assert rows.max() < R and cols.max() < C and rows.min() >= 0 and cols.min() >= 0
    key = rows * C + cols
    assert (np.diff(key) > 0).all()                 # sorted row-major, no duplicate pair
    assert (vals >= 0.5).all()


@pytest.mark.parametrize("n", [2049, 4096])
@pytest.mark.parametrize("name", S.LAYOUTS)
def test_layouts_are_what_they_are_named(name, n):
    rows, cols, vals, (R, C) = S.graph_layout(name, n)
    assert len(rows) == n and (np.diff(rows * C + cols) > 0).all()
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=R))])
    deg = np.diff(rowptr)
    if name == "leading_empty":
        assert (deg[:5] == 0).all() and deg[5:].sum() == n
    elif name == "trailing_empty":
        assert (rowptr[-7:] == n).all() and deg[-7] > 0   # several r with rowptr[r] == nnz
    elif name == "middle_empty":
        assert (deg[140:149] == 0).all() and deg[:140].sum() == n // 2
    elif name == "row_at_tile":
        r = int(np.searchsorted(rowptr, S.TILE))
        assert rowptr[r] == S.TILE and deg[r] > 0
    elif name == "one_row":
        assert R == 1 and deg[0] == n and C >= n
    else:
        assert R == int(name[4:])


def test_keep_masks_by_hand():
    assert S.keep_mask("all", 3).tolist() == [True, True, True]
    assert S.keep_mask("none", 3).tolist() == [False, False, False]
    assert S.keep_mask("first", 4).tolist() == [True, False, False, False]
    assert S.keep_mask("last", 4).tolist() == [False, False, False, True]
    assert S.keep_mask("first", 1).tolist() == [True] == S.keep_mask("last", 1).tolist()
    assert np.nonzero(S.keep_mask("round_heads", 600))[0].tolist() == [0, 256, 512]
    assert np.nonzero(S.keep_mask("round_heads", 256))[0].tolist() == [0]
    assert S.keep_mask("odd_tiles", 2048) is None
    m = S.keep_mask("odd_tiles", 4097)
    assert np.nonzero(m)[0].tolist() == list(range(2048, 4096))
    m = S.keep_mask("odd_tiles", 2049)
    assert np.nonzero(m)[0].tolist() == [2048]
    r = S.keep_mask("random", 4096)
    assert r.dtype == bool and 1800 < r.sum() < 2300
    assert np.array_equal(r, O.device_keep_mask(4096, 4096, 0.5))


def test_drop_reference_by_hand():
    # A = [[1, 0, 2], [0, 3, 0]]; drop the (0, 2) entry, keep rate 0.5
    rows, cols = np.array([0, 0, 1]), np.array([0, 2, 1])
    vals = np.array([1, 2, 3], np.float32)
    ref = S.drop_reference(rows, cols, vals, [True, False, True], 0.5, (2, 3))
    assert ref["rowptr"].tolist() == [0, 1, 2] and ref["col"].tolist() == [0, 1]
    assert ref["val"].tolist() == [2.0, 6.0] and ref["val"].dtype == np.float32
    assert ref["colptr"].tolist() == [0, 1, 2, 2] and ref["row_t"].tolist() == [0, 1]
    assert ref["val_t"].tolist() == [2.0, 6.0] and ref["nnz"] == 2
    # a column holding two rows comes out rows-ascending; binary matrix has no values
    rows, cols = np.array([0, 1, 1]), np.array([1, 0, 1])
    ref = S.drop_reference(rows, cols, None, [True, True, True], 0.3, (2, 2))
    assert ref["colptr"].tolist() == [0, 1, 3] and ref["row_t"].tolist() == [1, 0, 1]
    assert ref["val"] is None and ref["val_t"] is None
    # the division is float32's: 1 / 0.3f is not the float32 of 1 / 0.3
    ref = S.drop_reference(np.array([0]), np.array([0]), np.array([1], np.float32), [True], 0.3,
                           (1, 1))
    assert ref["val"][0] == np.float32(1) / np.float32(0.3)
    ref = S.drop_reference(rows, cols, None, [False, False, False], 0.3, (2, 2))
    assert ref["rowptr"].tolist() == [0, 0, 0] and ref["nnz"] == 0 and ref["col"].size == 0


def test_row_sums_f32_by_hand():
    s = S.row_sums_f32([0, 2, 2, 3], np.array([1e8, 1, 3], np.float32))
    assert s.dtype == np.float32 and s.tolist() == [1e8, 0.0, 3.0]   # 1e8 + 1 rounds to 1e8
    # the order is the entries': (1 + 1e8) - 1e8 = 0, while (1e8 - 1e8) + 1 = 1
    assert S.row_sums_f32([0, 3], np.array([1, 1e8, -1e8], np.float32)).tolist() == [0.0]
    assert S.row_sums_f32([0, 3], np.array([1e8, -1e8, 1], np.float32)).tolist() == [1.0]
    assert S.row_sums_f32([0, 0], np.zeros(0, np.float32)).tolist() == [0.0]


@pytest.mark.parametrize("n_rows", [63, 64, 65, 255, 256, 257, 1000])
def test_plan_degrees(n_rows):
    rng = np.random.default_rng(n_rows)
    d = S.plan_degrees(n_rows, "mixed", rng)
    assert d.shape == (n_rows,) and {16, 17, 24, 25, 400} <= set(d.tolist())
    heavy = np.nonzero(d > 16)[0]
    assert (heavy < 64).sum() >= 4 and d[60] == 400 and d[n_rows - 1] == 24
    assert d[n_rows - 2] == 25
    if n_rows > 256:
        assert ((heavy >= 192) & (heavy < 256)).any()       # last wave of the first block
        assert (heavy >= (n_rows - 1) // 256 * 256).any()   # last block
    light = S.plan_degrees(n_rows, "light", rng)
    assert light.max() == 16 and light.sum() > 16
    assert S.plan_degrees(n_rows, "heavy", rng).min() >= 17


def test_split_plan_by_hand():
    # degrees 17, 16, 25 at threshold 16, chunk 8: rows 0 and 2 are heavy, 3 and 4 chunks
    heavy, cptr, ch = O.split_plan(np.array([0, 17, 33, 58]), 16, 8)
    assert heavy.tolist() == [0, 2] and cptr.tolist() == [0, 3, 7]
    assert ch.tolist() == [0, 0, 0, 1, 1, 1, 1]
