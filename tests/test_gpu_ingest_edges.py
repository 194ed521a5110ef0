"""The device half of csrc/ingest.hip at its edges: ``ingest.remap_first_appearance``,
``ingest.coalesce`` and ``ingest.normalize_graph_mat`` bit-exact against the numpy restatements of
tests/_unique_ref.py (checked against the oracle's dict loop and scipy on the CPU by
tests/test_unique_ref.py): integers equal, floats compared as uint32. The cases sit on the two
radix sorts' key widths (``bits_for(2 * n)``, ``bits_for(n_rows * n_cols)``: counts that are an
exact power of two with the top key present), on the 256-thread block (kBlock) of every
per-element kernel and on the rowptr kernel's ``r > n_rows`` guard."""
import numpy as np
import pytest
import torch

from tests import _unique_ref as U

pytestmark = pytest.mark.gpu

REMAP = U.remap_cases()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- remap_first_appearance
@pytest.mark.parametrize("name", list(REMAP))
def test_remap_first_appearance(dev, name):
    """nN-*: n = 1, 2, 255, 256, 257 (kBlock), 1,024, 2^16 and 2^16 + 1 — with n a power of two
    the pad keys n + i of k_pad_segments reach 2n - 1, the top of ``bits_for(2 * n)`` in the
    second sort — with all keys distinct (no pad key), all equal (n - 1 pad keys, the largest
    present), n - 1 distinct (one pad key: 2n - 1) and 1 + n/2 distinct. extremes: INT64_MIN,
    -1, 0, INT64_MAX (the first sort is signed over 64 bits; the ids follow first appearance).
    descending: sort order and appearance order disagree everywhere. first-and-last: a key whose
    occurrences are the first and the last element (k_heads' ``i == 0``, the last segment)."""
    from hypergraph_diffusion_for_recommendation_amd.ingest import remap_first_appearance
    keys = REMAP[name]
    want_ids, want_uniq = U.remap_ref(keys)
    ids, uniq = remap_first_appearance(_t(keys, dev))
    assert ids.dtype == torch.int32 and uniq.dtype == torch.int64
    assert np.array_equal(uniq.cpu().numpy(), want_uniq)
    assert np.array_equal(ids.cpu().numpy(), want_ids)


def test_remap_empty(dev):
    """n = 0: the memset path — no ids, no keys."""
    from hypergraph_diffusion_for_recommendation_amd.ingest import remap_first_appearance
    ids, uniq = remap_first_appearance(torch.empty(0, dtype=torch.int64, device=dev))
    assert ids.numel() == 0 and uniq.numel() == 0


# ---------------------------------------------------------------- coalesce
def _check_coalesce(dev, rows, cols, n_rows, n_cols):
    from hypergraph_diffusion_for_recommendation_amd.ingest import coalesce
    want_rp, want_col, want_val = U.coalesce_ref(rows, cols, n_rows, n_cols)
    rp, col, val = coalesce(_t(rows, dev), _t(cols, dev), n_rows, n_cols)
    assert rp.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert np.array_equal(rp.cpu().numpy(), want_rp)
    assert np.array_equal(col.cpu().numpy(), want_col)
    assert np.array_equal(_bits(val.cpu().numpy()), _bits(want_val))
    return want_rp, want_col, want_val


SHAPES = [(256, 256), (1, 1 << 20), (1 << 20, 1), (3, 85), (257, 1), (65537, 65537)]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coalesce_shapes(dev, shape, n):
    """``bits_for(n_rows * n_cols)``: the cell count an exact power of two — (256, 256),
    (1, 2^20), (2^20, 1) — and 2^k ± 1 — (3, 85) = 255, (257, 1), (65,537, 65,537) — with the
    largest key (n_rows - 1, n_cols - 1) present (the only entry when n = 1) and (0, 0), both
    duplicated; n = 1, 255, 256, 257 on kBlock of k_keys2 / k_split_keys."""
    rows, cols = U.corner_coo(n, *shape, seed=n + shape[0])
    _, col, val = _check_coalesce(dev, rows, cols, *shape)
    if n >= 5:
        assert val[-1] >= 3.0 and val[0] >= 2.0 and col[-1] == shape[1] - 1 and col[0] == 0


def test_coalesce_keys_near_2_to_58(dev):
    """A (2^27, 2^31 - 2) shape: n_cols at the entry's int32 limit, keys up to about 2^58 through
    ``bits_for`` and the int64 divide of k_split_keys, and 2^27 + 1 threads of k_rowptr_runs.
    The issue's (2^31 - 2)^2 shape needs a 16 GiB rowptr; this one keeps it at 1 GiB (the suite's
    limit is about 1.2 GB per test), so the row count, not the column count, is the smaller.
    Not pinned as a result: key widths above about 2^58 and a row index near the int32 limit in
    k_split_keys / k_rowptr_runs. The rowptr stays on the device: its runs are compared slice by
    slice."""
    from hypergraph_diffusion_for_recommendation_amd.ingest import coalesce
    R, C = 1 << 27, (1 << 31) - 2
    mid = R // 2 + 1
    cells = [(0, 0), (R - 1, C - 1), (0, C - 1), (mid, 12345), (R - 1, 0), (0, 0), (R - 1, C - 1),
             (R - 1, C - 1), (mid, 12345), (mid, C - 1)]
    rows = np.array([c[0] for c in cells], dtype=np.int32)
    cols = np.array([c[1] for c in cells], dtype=np.int32)
    rr, want_col, want_val = U.coalesce_runs_ref(rows, cols, C)
    assert rr.tolist() == [0, 0, mid, mid, R - 1, R - 1]
    rp, col, val = coalesce(_t(rows, dev), _t(cols, dev), R, C)
    assert np.array_equal(col.cpu().numpy(), want_col)
    assert np.array_equal(_bits(val.cpu().numpy()), _bits(want_val))
    assert want_val.tolist() == [2, 1, 2, 1, 1, 3]
    assert rp.numel() == R + 1
    assert rp[[0, 1, mid, mid + 1, R - 1, R]].tolist() == [0, 2, 2, 4, 4, 6]
    for a, b, v in ((0, 1, 0), (1, mid + 1, 2), (mid + 1, R, 4), (R, R + 1, 6)):
        assert bool((rp[a:b] == v).all()), (a, b, v)


def _layout(name, n_rows, n_cols, rng):
    per = 4
    if name == "row0":
        rows = np.zeros(3 * n_rows, dtype=np.int64)
    elif name == "last_row":
        rows = np.full(3 * n_rows, n_rows - 1, dtype=np.int64)
    elif name == "one_per_row":
        rows = rng.permutation(n_rows)
    elif name == "empty_start_middle_end":
        live = np.r_[5:n_rows // 2 - 3, n_rows // 2 + 4:n_rows - 6]
        rows = rng.permutation(np.repeat(live, per))
    else:
        raise KeyError(name)
    return rows.astype(np.int32), rng.integers(0, n_cols, size=len(rows)).astype(np.int32)


@pytest.mark.parametrize("n_rows", [255, 256, 257])
@pytest.mark.parametrize("layout", ["row0", "last_row", "one_per_row", "empty_start_middle_end"])
def test_coalesce_row_layouts(dev, layout, n_rows):
    """k_rowptr_runs: n_rows + 1 = 256 and 257 threads (``r > n_rows``, the r == n_rows thread
    the last of a block and the first of the next), with every entry in row 0 (rowptr[1:] all
    nnz), every entry in the last row (rowptr[:n_rows] all 0), one entry per row, and empty rows
    at the start, in the middle and at the end (the binary search's lo == hi ends)."""
    rng = np.random.default_rng(n_rows)
    rows, cols = _layout(layout, n_rows, 40, rng)
    rp, _, _ = _check_coalesce(dev, rows, cols, n_rows, 40)
    if layout == "empty_start_middle_end":
        assert rp[5] == 0 and rp[-1] == rp[-7] and rp[n_rows // 2 - 3] == rp[n_rows // 2 + 4]


@pytest.mark.parametrize("mult", [1, 2, 255])
def test_coalesce_multiplicity(dev, mult):
    """One cell entered 1, 2 and 255 times among others: the run-length count becomes the float32
    value (``static_cast<float>(counts[i])`` in k_split_keys)."""
    rng = np.random.default_rng(mult)
    rows = np.concatenate([rng.integers(0, 9, 300), np.full(mult, 4)]).astype(np.int32)
    cols = np.concatenate([rng.integers(0, 50, 300), np.full(mult, 50)]).astype(np.int32)
    p = rng.permutation(len(rows))
    rp, col, val = _check_coalesce(dev, rows[p], cols[p], 9, 51)
    assert val[rp[5] - 1] == mult and col[rp[5] - 1] == 50


def test_coalesce_multiplicity_past_float32_integers(dev):
    """One cell entered 2^24 + 1 times (n = 2^24 + 257): the int32 count 16,777,217 is not a
    float32; the stored value is 16,777,216.0 — what scipy's float32 sum of that many ones gives
    as well — and equals coalesce_ref computed in float32."""
    from hypergraph_diffusion_for_recommendation_amd.ingest import coalesce
    mult, extra = (1 << 24) + 1, 256
    rng = np.random.default_rng(24)
    er = rng.integers(0, 7, extra).astype(np.int32)
    ec = rng.integers(0, 30, extra).astype(np.int32)
    rows = torch.full((mult + extra,), 3, dtype=torch.int32, device=dev)
    cols = torch.full((mult + extra,), 30, dtype=torch.int32, device=dev)
    rows[::mult // extra + 1][:extra] = _t(er, dev)  # the others spread through the run
    cols[::mult // extra + 1][:extra] = _t(ec, dev)
    rp, col, val = coalesce(rows, cols, 7, 31)
    want_rp, want_col, want_val = U.coalesce_ref(rows.cpu().numpy(), cols.cpu().numpy(), 7, 31)
    assert np.array_equal(rp.cpu().numpy(), want_rp)
    assert np.array_equal(col.cpu().numpy(), want_col)
    assert np.array_equal(_bits(val.cpu().numpy()), _bits(want_val))
    at = int(want_rp[4]) - 1  # (3, 30): the last cell of row 3
    assert want_col[at] == 30 and float(val[at]) == 16777216.0
    assert float(val.sum(dtype=torch.float64)) == mult + extra - 1


def test_coalesce_empty(dev):
    """n = 0: rowptr all zero, nnz 0 (the memset path), at n_rows + 1 = 257."""
    from hypergraph_diffusion_for_recommendation_amd.ingest import coalesce
    e = torch.empty(0, dtype=torch.int32, device=dev)
    rp, col, val = coalesce(e, e, 256, 7)
    assert rp.numel() == 257 and not rp.any() and col.numel() == 0 and val.numel() == 0


# ---------------------------------------------------------------- normalize_graph_mat
def _csr(rng, degs, n_cols):
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n_cols, size=int(d), replace=False))
                          for d in degs]).astype(np.int32)
    val = rng.integers(1, 5, size=len(col)).astype(np.float32)  # counts: exact float32 row sums
    return rowptr, col, val


NORM = {
    "rect255": (255, 300), "rect256": (256, 300), "rect257": (257, 300),
    "square255": (255, 255), "square256": (256, 256), "square257": (257, 257),
    "rect-long-row": (256, 10001), "square-long-row": (10003, 10003),
}


@pytest.mark.parametrize("name", list(NORM))
def test_normalize_graph_mat(dev, name):
    """k_normalize_values: one thread per row, n_rows = 255, 256, 257 (``r >= n_rows`` on
    kBlock); square (``(d_r · v) · d_c``) and rectangular (``d_r · v``, col_scale null); rows
    with no entry (row sum 0: the scale is 0, not inf or NaN); a row with one entry and a row
    with 10,000. The scales are the numpy ``power`` call of the wrapper on the exact integer row
    sums (1 to 4·10^4, so every scale and product is a normal float32)."""
    from hypergraph_diffusion_for_recommendation_amd.ingest import normalize_graph_mat
    n_rows, n_cols = NORM[name]
    rng = np.random.default_rng(n_rows + n_cols)
    degs = rng.integers(1, 12, size=n_rows)
    degs[[0, n_rows // 2, n_rows - 1]] = 0
    degs[[1, n_rows - 2]] = 1
    if "long" in name:
        degs[7] = 10000
    rowptr, col, val = _csr(rng, degs, n_cols)
    square = n_rows == n_cols
    rs = np.bincount(np.repeat(np.arange(n_rows), degs), weights=val, minlength=n_rows)
    assert rs.max() < 2 ** 24  # integers: the float32 sum is exact in any order
    rs = rs.astype(np.float32).reshape(-1, 1)
    with np.errstate(divide="ignore"):
        d = np.power(rs, -0.5 if square else -1).flatten()
    d[np.isinf(d)] = 0.
    want = U.normalize_ref(rowptr, col, val, d, d if square else None)
    assert np.isfinite(want).all() and d[0] == 0 and (d[degs > 0] >= 2.4e-5).all()
    got = normalize_graph_mat(_t(rowptr, dev), _t(col, dev), _t(val, dev), (n_rows, n_cols))
    assert got.dtype == torch.float32
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
