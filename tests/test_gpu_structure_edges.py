"""The structure primitives (csrc/structure.hip) at their tile, wave and block boundaries.

Every hop runs over arrays these kernels build — row pointers, the CSC permutation, split plans,
drop-edge compaction, byte-mask gathers — and a wrong one does not crash: it changes which rows a
hop sums. tests/test_gpu_structure.py pins each at one comfortable shape; here the entry counts sit
on the 64-lane wave, the 256-entry round, the 2,048-entry tile and the 1,024-tile scan, the masks
on the first and last entry of each, the row counts on the 256-thread block, and the rows are empty
where a guard has to notice. Inputs and the two numpy restatements the oracle lacks are
tests/_structure_ref.py (checked on the CPU by tests/test_structure_ref.py).

Every comparison is bit-exact against numpy (integers equal, floats as uint32) except the hop over
a dropped child of a parent with split rows, which is held to the project's 1e-5·Σ|terms|
(tests/_util.assert_close) against the float64 oracle.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests import _structure_ref as S
from tests._util import assert_close

pytestmark = pytest.mark.gpu

N_LIST = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 2 * 2048 + 1)
eq = np.testing.assert_array_equal


def _np(t):
    return t.cpu().numpy()


def eq_bits(got, ref, what=""):
    """float32 arrays equal bit for bit (a NaN equals itself, -0.0 differs from 0.0)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == np.float32 and ref.dtype == np.float32, (what, got.dtype, ref.dtype)
    eq(got.view(np.uint32), ref.view(np.uint32), err_msg=what)


def _inc(rows, cols, vals, shape, dev, **kw):
    from hypergraph_diffusion_for_recommendation_amd import Incidence
    idx = torch.from_numpy(np.stack([rows, cols]).astype(np.int64))
    v = None if vals is None else torch.from_numpy(np.asarray(vals, dtype=np.float32))
    return Incidence.from_coo(idx, v, shape, device=dev, **kw)


@functools.lru_cache(maxsize=None)
def _parent(kind, n, weighted, dev):
    """The graph of exactly ``n`` entries (``kind`` 'exact' or a row layout of _structure_ref) and
    its Incidence, built once: a structure is immutable and every drop leaves its parent alone."""
    g = S.graph_exact(n) if kind == "exact" else S.graph_layout(kind, n)
    rows, cols, vals, shape = g
    inc = _inc(rows, cols, vals if weighted else None, shape, dev)
    assert inc.nnz == n and inc.coo_sorted and inc.perm_t is not None
    return g, inc


def _assert_dropped(d, ref, weighted, what):
    """An exact drop equals the kept COO rebuilt from scratch, both orientations."""
    k = ref["nnz"]
    assert d.nnz == k and d.csr.nnz == k and d.csc.nnz == k, what
    for o, ptr, idx in ((d.csr, "rowptr", "col"), (d.csc, "colptr", "row_t")):
        assert o.col.numel() == k and o.col.dtype == torch.int32, what
        eq(_np(o.rowptr), ref[ptr], err_msg=f"{what} {ptr}")
        eq(_np(o.col), ref[idx], err_msg=f"{what} {idx}")
    if weighted:
        assert d.val.numel() == k and d.val_t.numel() == k, what
        eq_bits(_np(d.val), ref["val"], f"{what} val")
        eq_bits(_np(d.val_t), ref["val_t"], f"{what} val_t")
    else:
        assert d.val is None and d.val_t is None, what


# ---- 1. tiled compaction: hgd_dropedge_structure / _compact / _fill_tail -------------------------
WK = [pytest.param(False, 0.7, id="binary"), pytest.param(True, 0.3, id="w-keep0.3"),
      pytest.param(True, 0.7, id="w-keep0.7"), pytest.param(True, 1.0, id="w-keep1.0")]
N_MASK = [(n, m) for n in N_LIST for m in S.MASKS if S.keep_mask(m, n) is not None]


@pytest.mark.parametrize("weighted,keep", WK)
@pytest.mark.parametrize("n,mask_name", N_MASK)
def test_drop_exact_counts_and_masks(dev, n, mask_name, weighted, keep):
    """Incidence.drop at entry counts on the wave, round and tile boundaries under masks that keep
    only the first or last entry of a tile, a round or the whole array."""
    (rows, cols, vals, shape), inc = _parent("exact", n, weighted, dev)
    mask = S.keep_mask(mask_name, n)
    d = inc.drop(torch.from_numpy(mask).to(dev), keep)
    ref = S.drop_reference(rows, cols, vals if weighted else None, mask, keep, shape)
    _assert_dropped(d, ref, weighted, f"n={n} mask={mask_name} keep={keep}")


@pytest.mark.parametrize("mask_name", ["all", "none", "last", "odd_tiles", "random"])
@pytest.mark.parametrize("n", [2049, 4096])
@pytest.mark.parametrize("layout", S.LAYOUTS)
def test_drop_row_layouts(dev, layout, n, mask_name):
    """Row pointers of the dropped structure where rows are empty at the start, the end (rowptr[r]
    == nnz, the else-branch of k_rowptr_tiles) or in the middle, a row starts on a tile boundary,
    one row holds everything, and the r == n_rows thread ends or begins a block."""
    (rows, cols, vals, shape), inc = _parent(layout, n, True, dev)
    mask = S.keep_mask(mask_name, n)
    d = inc.drop(torch.from_numpy(mask).to(dev), 0.7)
    ref = S.drop_reference(rows, cols, vals, mask, 0.7, shape)
    _assert_dropped(d, ref, True, f"{layout} n={n} mask={mask_name}")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mask_name", ["all", "none", "random"])
@pytest.mark.parametrize("n", N_LIST)
def test_drop_capacity(dev, n, mask_name, weighted):
    """drop(capacity=True): arrays of the parent's length, the exact drop's entries and row
    pointers, and zeros in [kept, nnz)."""
    (rows, cols, vals, shape), inc = _parent("exact", n, weighted, dev)
    mask = S.keep_mask(mask_name, n)
    d = inc.drop(torch.from_numpy(mask).to(dev), 0.7, capacity=True)
    ref = S.drop_reference(rows, cols, vals if weighted else None, mask, 0.7, shape)
    k = ref["nnz"]
    what = f"n={n} mask={mask_name}"
    for o, ptr, idx in ((d.csr, "rowptr", "col"), (d.csc, "colptr", "row_t")):
        assert o.col.numel() == n and o.nnz == n, what
        eq(_np(o.rowptr), ref[ptr], err_msg=f"{what} {ptr}")
        got = _np(o.col)
        eq(got[:k], ref[idx], err_msg=f"{what} {idx}")
        eq(got[k:], np.zeros(n - k, np.int32), err_msg=f"{what} {idx} tail")
    if weighted:
        for got, name in ((_np(d.val), "val"), (_np(d.val_t), "val_t")):
            assert got.shape == (n,), what
            eq_bits(got[:k], ref[name], f"{what} {name}")
            eq_bits(got[k:], np.zeros(n - k, np.float32), f"{what} {name} tail")
    else:
        assert d.val is None and d.val_t is None


BIG_N = 1024 * 2048 + 1  # 1,025 tiles: k_tile_scan sums two tiles per thread


@pytest.fixture(scope="module")
def big_graph():
    """5,000 x 3,000, exactly BIG_N entries, random degrees, the first three rows empty; the mask
    of the device draw at keep 0.6."""
    rng = np.random.default_rng(77)
    degs = np.concatenate([np.zeros(3, np.int64), S.split_count(rng, BIG_N, 4997)])
    rows, cols = S.coo_from_degrees(rng, degs, 3000)
    vals = (rng.random(BIG_N) + 0.5).astype(np.float32)
    assert len(rows) == BIG_N and rows[0] == 3
    return rows, cols, vals, (5000, 3000), O.device_keep_mask(5, BIG_N, 0.6)


@pytest.mark.parametrize("weighted", [False, True])
def test_drop_above_1024_tiles(dev, big_graph, weighted):
    rows, cols, vals, shape, mask = big_graph
    assert S.TILE * 1024 < len(rows) <= S.TILE * 1025
    inc = _inc(rows, cols, vals if weighted else None, shape, dev)
    d = inc.drop(torch.from_numpy(mask).to(dev), 0.6)
    ref = S.drop_reference(rows, cols, vals if weighted else None, mask, 0.6, shape)
    _assert_dropped(d, ref, weighted, "1,025 tiles")


def test_drop_at_exactly_1024_tiles(dev, big_graph):
    rows, cols, _, shape, mask = big_graph
    rows, cols, mask = rows[:-1], cols[:-1], mask[:-1]
    assert len(rows) == S.TILE * 1024
    inc = _inc(rows, cols, None, shape, dev)
    d = inc.drop(torch.from_numpy(mask).to(dev), 0.6)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[mask], minlength=shape[0]))])
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols[mask], minlength=shape[1]))])
    eq(_np(d.csr.rowptr), rowptr)
    eq(_np(d.csc.rowptr), colptr)
    assert d.nnz == int(mask.sum())


@pytest.mark.parametrize("mask_name", ["random", "none", "all"])
@pytest.mark.parametrize("n", N_LIST)
def test_drop_edges_coo(dev, n, mask_name):
    """drop_edges (hgd_dropedge_compact, the int64 COO writer) against O.dropedge."""
    from hypergraph_diffusion_for_recommendation_amd.incidence import drop_edges
    rows, cols, vals, _ = S.graph_exact(n)
    mask = S.keep_mask(mask_name, n)
    idx, v = drop_edges(torch.from_numpy(np.stack([rows, cols])).to(dev),
                        torch.from_numpy(vals).to(dev), torch.from_numpy(mask).to(dev), 0.7)
    ref_idx, ref_v = O.dropedge(np.stack([rows, cols]), vals, mask, 0.7)
    assert tuple(idx.shape) == ref_idx.shape and idx.dtype == torch.int64
    eq(_np(idx), ref_idx)
    eq_bits(_np(v), ref_v)


# ---- 2. hgd_gather_u8 ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 1023, 1024, 1025, 1027])
def test_gather_u8_tail_and_guard(dev, n):
    """out[i] = src[perm[i]] at sizes around the four-per-thread body and its tail loop; nothing
    past out[n - 1] is written."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    rng = np.random.default_rng(n)
    src = rng.integers(0, 256, n).astype(np.uint8)
    src[0], src[-1] = 0, 255
    perm = rng.permutation(n).astype(np.int32)
    src_t = torch.from_numpy(src).to(dev)
    perm_t = torch.from_numpy(perm).to(dev)
    assert perm_t.data_ptr() % 16 == 0
    out = torch.full((n + 8,), 0xAB, dtype=torch.uint8, device=dev)
    nat.check(lib.hgd_gather_u8(src_t.data_ptr(), perm_t.data_ptr(), n, out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "hgd_gather_u8")
    got = _np(out)
    eq(got[:n], src[perm])
    eq(got[n:], np.full(8, 0xAB, np.uint8))


@pytest.mark.parametrize("rem", [1, 2, 3])
def test_masked_view_csc_mask(dev, rem):
    """Incidence.masked: the CSC-order mask is mask[perm_t], with an entry count that leaves the
    byte gather a tail of 1, 2 and 3."""
    n = 1024 + rem
    (rows, cols, _, (R, C)), inc = _parent("exact", n, False, dev)
    assert inc.nnz % 4 == rem
    mask = S.keep_mask("random", n, seed=rem)
    view = inc.masked(torch.from_numpy(mask).to(dev), 0.5)
    rowptr, col, _, _ = O.csr_from_coo(rows, cols, R)
    perm = O.transpose_csr(rowptr, col, C)[3]
    eq(_np(inc.perm_t), perm)
    eq(_np(view.csr.mask), mask.astype(np.uint8))
    eq(_np(view.csc.mask), mask[perm].astype(np.uint8))


# ---- 3. split plan on the device: hgd_split_plan_count / _build ------------------------------
PLAN_ROWS = (63, 64, 65, 255, 256, 257, 1000)
PLAN_COLS = 450


def _plan_graph(n_rows, variant, skew=False):
    rng = np.random.default_rng(31 * n_rows + len(variant) + skew)
    degs = S.plan_degrees(n_rows, variant, rng)
    p = None
    if skew:  # the first columns collect most rows: heavy columns on the CSC side
        p = 1.0 / (1.0 + np.arange(PLAN_COLS))
        p /= p.sum()
    rows, cols = S.coo_from_degrees(rng, degs, PLAN_COLS, p)
    vals = rng.standard_normal(len(rows)).astype(np.float32)
    return rows, cols, vals, degs


def _assert_plan(o, ptr, what):
    heavy, cptr, ch = O.split_plan(ptr, 16, 8)
    assert o.n_heavy == len(heavy), what
    if len(heavy) == 0:
        assert o.plan.threshold == 0 and o._plan_arrays == (), what
        return
    p = o.plan
    assert (p.threshold, p.chunk, p.n_heavy, p.n_chunks) == (16, 8, len(heavy), len(ch)), what
    ha, hc, chh = o._plan_arrays
    eq(_np(ha), heavy, err_msg=f"{what} heavy_rows")
    eq(_np(hc), cptr, err_msg=f"{what} heavy_cptr")
    eq(_np(chh), ch, err_msg=f"{what} chunk_heavy")


@pytest.mark.parametrize("variant", ["mixed", "light", "heavy"])
@pytest.mark.parametrize("n_rows", PLAN_ROWS)
def test_plan_rows(dev, n_rows, variant):
    """The device split plan over one wave, a full block, a block and one row, and four blocks:
    heavy rows in the first wave, the last wave of a block, the last block and as the last row;
    none heavy (the plan is off); every row heavy."""
    rows, cols, vals, degs = _plan_graph(n_rows, variant)
    inc = _inc(rows, cols, vals, (n_rows, PLAN_COLS), dev, split_threshold=16, split_chunk=8)
    rowptr = np.concatenate([[0], np.cumsum(degs)])
    eq(_np(inc.csr.rowptr), rowptr)
    n_heavy = int((degs > 16).sum())
    assert n_heavy == {"light": 0, "heavy": n_rows}.get(variant, n_heavy)
    _assert_plan(inc.csr, rowptr, f"rows={n_rows} {variant}")
    if variant == "light":
        assert inc.csr.plan.threshold == 0


@pytest.mark.parametrize("variant", ["mixed", "light", "heavy"])
@pytest.mark.parametrize("n_cols", PLAN_ROWS)
def test_plan_columns(dev, n_cols, variant):
    """The same plans on the CSC side: a graph whose COLUMNS carry the skewed degrees."""
    a, b, vals, degs = _plan_graph(n_cols, variant)
    rows, cols = b, a  # the transpose, put back into row-major order
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    inc = _inc(rows, cols, vals, (PLAN_COLS, n_cols), dev, split_threshold=16, split_chunk=8)
    colptr = np.concatenate([[0], np.cumsum(degs)])
    eq(_np(inc.csc.rowptr), colptr)
    _assert_plan(inc.csc, colptr, f"cols={n_cols} {variant}")
    _assert_plan(inc.csr, _np(inc.csr.rowptr), f"cols={n_cols} {variant} csr side")


def test_plan_of_dropped_child_and_its_hop(dev):
    """Incidence.drop on a parent with split rows rebuilds the child's plans: some heavy rows stay
    heavy, some turn light, one is emptied; the hop over the child (both orientations, d = 64) is
    the float64 oracle's within 1e-5·Σ|terms|."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    R, C, d = 257, PLAN_COLS, 64
    rows, cols, vals, degs = _plan_graph(R, "mixed", skew=True)
    n = len(rows)
    inc = _inc(rows, cols, vals, (R, C), dev, split_threshold=16, split_chunk=8)
    assert inc.coo_sorted and inc.csr.n_heavy and inc.csc.n_heavy
    rowptr = np.concatenate([[0], np.cumsum(degs)])
    mask = O.device_keep_mask(3, n, 0.5).copy()
    for r, k in ((60, 400), (1, 3), (5, 0), (256, 20)):  # heavy, light, empty, heavy
        mask[rowptr[r]:rowptr[r + 1]] = False
        mask[rowptr[r]:rowptr[r] + k] = True
    child = inc.drop(torch.from_numpy(mask).to(dev), 0.5)
    ref = S.drop_reference(rows, cols, vals, mask, 0.5, (R, C))
    cdeg = np.diff(ref["rowptr"])
    assert degs[[60, 1, 5, 256]].tolist() == [400, 17, 24, 24]
    assert cdeg[[60, 1, 5, 256]].tolist() == [400, 3, 0, 20]
    _assert_dropped(child, ref, True, "child of a heavy parent")
    _assert_plan(child.csr, ref["rowptr"], "child csr")
    _assert_plan(child.csc, ref["colptr"], "child csc")
    assert 0 < child.csr.n_heavy < inc.csr.n_heavy
    assert 0 < child.csc.n_heavy < inc.csc.n_heavy
    rng = np.random.default_rng(9)
    for o, val, ptr, idx, v, n_src in ((child.csr, child.val, "rowptr", "col", "val", C),
                                       (child.csc, child.val_t, "colptr", "row_t", "val_t", R)):
        X = rng.standard_normal((n_src, d)).astype(np.float32)
        Y = spmm_csr(o, torch.from_numpy(X).to(dev), val)
        want = O.spmm_csr(ref[ptr], ref[idx], X, ref[v])
        mag = O.spmm_csr(ref[ptr], ref[idx], X, ref[v], absolute=True)
        assert_close(_np(Y), want, mag, what=f"hop over the child's {ptr}")


# ---- 4. Incidence.from_coo for unsorted input ------------------------------------------------
def _assert_from_coo(inc, r, c, v, shape, what):
    from hypergraph_diffusion_for_recommendation_amd.incidence import expand_rows
    R, C = shape
    rowptr, col, vv, _ = O.csr_from_coo(r, c, R, v)
    colptr, rows_t, vt, perm = O.transpose_csr(rowptr, col, C, vv)
    assert inc.nnz == len(r), what
    eq(_np(inc.csr.rowptr), rowptr, err_msg=f"{what} rowptr")
    eq(_np(inc.csr.col), col, err_msg=f"{what} col")
    eq_bits(_np(inc.val), vv, f"{what} val")  # the stable order inside a row
    eq(_np(inc.csc.rowptr), colptr, err_msg=f"{what} colptr")
    eq(_np(inc.csc.col), rows_t, err_msg=f"{what} row_t")
    eq_bits(_np(inc.val_t), vt, f"{what} val_t")
    eq(_np(inc.perm_t), perm, err_msg=f"{what} perm_t")
    eq(_np(expand_rows(inc.csr.rowptr, inc.nnz)), np.sort(r), err_msg=f"{what} expand_rows")
    assert inc.coo_sorted == bool((np.diff(r) >= 0).all()), what


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 3), (256, 257), (257, 256),
                                   (65536, 5), (65537, 5), (5, 65536), (5, 65537)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_from_coo_unsorted_key_bits(dev, shape):
    """3,000 unsorted entries with duplicates at key counts of 1, a power of two and a power of two
    plus one, the largest row and column id present: the radix sort's top key bit."""
    R, C = shape
    rng = np.random.default_rng(R * 7 + C)
    m = 3000
    r = rng.integers(0, R, m)
    c = rng.integers(0, C, m)
    r[100:110], c[100:110] = r[:10], c[:10]  # duplicate pairs stay separate entries
    r[[7, 2000]] = R - 1
    c[[11, 2500]] = C - 1
    v = rng.standard_normal(m).astype(np.float32)
    assert r.max() == R - 1 and c.max() == C - 1
    _assert_from_coo(_inc(r, c, v, shape, dev), r, c, v, shape, f"{R}x{C}")


@pytest.mark.parametrize("variant", ["sorted_but_last", "sorted", "one_row", "rows_0_and_256"])
def test_from_coo_order_variants(dev, variant):
    R, C, m = 257, 256, 3000
    rng = np.random.default_rng(len(variant))
    c = rng.integers(0, C, m)
    c[5] = C - 1
    if variant in ("sorted_but_last", "sorted"):
        r = np.sort(rng.integers(0, R, m))
        r[-2] = R - 1
        r[-1] = 0 if variant == "sorted_but_last" else R - 1
    elif variant == "one_row":
        r = np.full(m, R - 1)
    else:
        r = rng.choice([0, R - 1], m)
    v = rng.standard_normal(m).astype(np.float32)
    inc = _inc(r, c, v, (R, C), dev, rows_sorted=None)
    assert inc.coo_sorted == (variant in ("sorted", "one_row"))  # the no-sort path
    _assert_from_coo(inc, r, c, v, (R, C), variant)
    if variant == "rows_0_and_256":
        assert (np.diff(_np(inc.csr.rowptr))[1:-1] == 0).all()


def test_from_coo_empty_and_its_drop(dev):
    from hypergraph_diffusion_for_recommendation_amd.incidence import expand_rows
    z = np.zeros(0, np.int64)
    inc = _inc(z, z, np.zeros(0, np.float32), (5, 9), dev)
    eq(_np(inc.csr.rowptr), np.zeros(6, np.int64))
    eq(_np(inc.csc.rowptr), np.zeros(10, np.int64))
    assert inc.nnz == 0 and inc.perm_t.numel() == 0 and inc.csr.col.numel() == 0
    assert expand_rows(inc.csr.rowptr, 0).numel() == 0
    for capacity in (False, True):
        d = inc.drop(torch.zeros(0, dtype=torch.bool, device=dev), 0.5, capacity=capacity)
        eq(_np(d.csr.rowptr), np.zeros(6, np.int64))
        eq(_np(d.csc.rowptr), np.zeros(10, np.int64))
        assert d.nnz == 0 and d.csr.col.numel() == 0 and d.csc.col.numel() == 0
        assert d.val.numel() == 0 and d.val_t.numel() == 0


# ---- 5. degree scales: hgd_degree_scale ------------------------------------------------------
@pytest.mark.parametrize("n", [2049, 4096])
@pytest.mark.parametrize("layout", S.LAYOUTS)
def test_degree_scales_on_row_layouts(dev, layout, n):
    """'mean', 'sym', 'wmean' and 'wsym' over rows and columns of the layouts with empty rows at
    the start, the end and in the middle: exactly 0 for an empty row, O.degree_scale rounded to
    float32 elsewhere, the weighted sums taken in float32 in edge order."""
    (rows, cols, vals, (R, C)), inc = _parent(layout, n, True, dev)
    rowptr, col, v, _ = O.csr_from_coo(rows, cols, R, vals)
    colptr, _, vt, _ = O.transpose_csr(rowptr, col, C, v)
    for side, ptr, w in (("row", rowptr, v), ("col", colptr, vt)):
        deg = np.diff(ptr)
        wdeg = S.row_sums_f32(ptr, w)
        assert ((wdeg == 0) == (deg == 0)).all()  # the weights are positive
        for kind, p in (("mean", -1.0), ("sym", -0.5)):
            what = f"{layout} n={n} {side}"
            got = _np(inc.scale(side, kind))
            eq_bits(got, O.degree_scale(deg, p).astype(np.float32), f"{what} {kind}")
            eq_bits(got[deg == 0], np.zeros(int((deg == 0).sum()), np.float32), what)
            got = _np(inc.scale(side, "w" + kind))
            eq_bits(got, O.degree_scale(wdeg.astype(np.float64), p).astype(np.float32),
                    f"{what} w{kind}")
            eq_bits(got[deg == 0], np.zeros(int((deg == 0).sum()), np.float32), what)


# ---- 6. dense_threshold ----------------------------------------------------------------------
def _dense_matrix(shape, fill, seed):
    """``mixed``: zeros, -0.0, negatives, entries exactly 0.25, one NaN, an all-zero row and an
    all-kept row where the shape has room; ``none``: nothing any mode keeps; ``all``: everything."""
    rng = np.random.default_rng(seed)
    if fill == "none":
        return np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0))
    if fill == "all":
        return (rng.random(shape) + 0.5).astype(np.float32)
    H = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, -1.0, 0.75, 0.1, -0.25], np.float32), size=shape)
    if H.shape[0] >= 3:
        H[0] = 0.0
        H[1] = 0.9
    if H.size >= 3:
        H.reshape(-1)[H.size - 2] = np.nan
    return H


def _assert_dense(H, Hdev, thresh, nonzero, what):
    from hypergraph_diffusion_for_recommendation_amd.incidence import dense_threshold
    rowptr, cols, vals = dense_threshold(Hdev, thresh, nonzero=nonzero, values=True)
    Ht = torch.from_numpy(np.ascontiguousarray(H))
    want = torch.nonzero(Ht) if nonzero else torch.nonzero(Ht > thresh)
    wr, wc = want[:, 0].numpy(), want[:, 1].numpy()
    # numpy states the same rule: NaN != 0 is kept, -0.0 != 0 is not, and > keeps neither
    nr, nc = np.nonzero(H != 0) if nonzero else np.nonzero(H > np.float32(thresh))
    eq(wr, nr, err_msg=what)
    eq(wc, nc, err_msg=what)
    got_ptr = _np(rowptr)
    eq(got_ptr, np.concatenate([[0], np.cumsum(np.bincount(wr, minlength=H.shape[0]))]),
       err_msg=f"{what} rowptr")
    assert cols.dtype == torch.int32 and cols.numel() == len(wc), what
    eq(_np(cols), wc, err_msg=f"{what} cols")
    eq_bits(_np(vals), np.ascontiguousarray(H[wr, wc]), f"{what} values")
    rowptr2, cols2 = dense_threshold(Hdev, thresh, nonzero=nonzero)
    assert torch.equal(rowptr2, rowptr) and torch.equal(cols2, cols), what
    return wr, wc


MODES = [pytest.param(0.0, False, id="gt0"), pytest.param(0.25, False, id="gt0.25"),
         pytest.param(0.0, True, id="nonzero")]


@pytest.mark.parametrize("fill", ["mixed", "none", "all"])
@pytest.mark.parametrize("thresh,nonzero", MODES)
@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 128, 129])
@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 9])
def test_dense_threshold_modes(dev, n_rows, n_cols, thresh, nonzero, fill):
    """torch.nonzero(H > thresh) / torch.nonzero(H) at column counts around the 64-lane sweep and
    row counts around the four rows of a workgroup."""
    H = _dense_matrix((n_rows, n_cols), fill, n_rows * 131 + n_cols)
    what = f"{n_rows}x{n_cols} thresh={thresh} nonzero={nonzero} {fill}"
    wr, wc = _assert_dense(H, torch.from_numpy(H).to(dev), thresh, nonzero, what)
    kept = np.zeros(H.shape, bool)
    kept[wr, wc] = True
    if fill == "none":
        assert not kept.any(), what
    elif fill == "all":
        assert kept.all(), what
    else:
        assert not kept[H == np.float32(thresh)].any(), what  # equal to the threshold: dropped
        assert not kept[H == 0].any(), what                   # -0.0 included, in every mode
        for special in (np.isnan(H), H < 0):                  # kept by != 0 only
            assert (kept[special] == nonzero).all(), what


@pytest.mark.parametrize("thresh,nonzero", MODES)
def test_dense_threshold_strided_views(dev, thresh, nonzero):
    """A row-strided view (stride(0) = 130 over 65 columns) is read in place and a column-strided
    one through a contiguous copy: both give the contiguous matrix's result."""
    H = _dense_matrix((9, 130), "mixed", 5)
    Hdev = torch.from_numpy(H).to(dev)
    view = Hdev[:, :65]
    assert view.stride() == (130, 1) and not view.is_contiguous()
    _assert_dense(H[:, :65], view, thresh, nonzero, "row-strided view")
    view = Hdev[:, ::2]
    assert view.stride() == (130, 2)
    _assert_dense(H[:, ::2], view, thresh, nonzero, "column-strided view")


# ---- 7. device graph build, the degenerate inputs --------------------------------------------
def _degenerate_records(case):
    rng = np.random.default_rng(17)
    if case == "one_record":
        return np.array([5], np.int64), np.array([9], np.int64)
    if case == "one_pair_5000_times":
        return np.full(5000, -12345, np.int64), np.full(5000, 678, np.int64)
    if case == "all_distinct":
        return (rng.permutation(5000).astype(np.int64) * 7 - 3,
                rng.permutation(5000).astype(np.int64) * 11 + 1)
    assert case == "int64_extremes"
    ids = np.array([-2 ** 63, 2 ** 63 - 1, 0, -1, 5, -2 ** 63 + 1, 2 ** 63 - 2], np.int64)
    users = rng.choice(ids, 400)
    users[:3] = (2 ** 63 - 1, -2 ** 63, 0)
    return users, rng.integers(0, 40, 400).astype(np.int64)


@pytest.mark.parametrize("case", ["one_record", "one_pair_5000_times", "all_distinct",
                                  "int64_extremes"])
def test_interaction_graph_degenerate_inputs(dev, case):
    """InteractionGraph against the dict-and-scipy restatement of tests/test_gpu_ingest.py, with
    the assertions of test_interaction_graph_matches_reference."""
    from hypergraph_diffusion_for_recommendation_amd.ingest import InteractionGraph
    from tests.test_gpu_ingest import _canon, _oracle, _same_structure
    users, items = _degenerate_records(case)
    g = InteractionGraph(users, items, dev)
    user, item, ui, ii, adj, norm, R, normR = _oracle(users, items)
    assert g.n_users == len(user) and g.n_items == len(item)
    assert g.user_raw.cpu().tolist() == list(user.keys())
    assert g.item_raw.cpu().tolist() == list(item.keys())
    eq(_np(g.user_idx), ui)
    eq(_np(g.item_idx), ii)
    counts = _same_structure(g.ui_adj, adj)
    eq(_np(g.ui_adj.val), counts)
    vals = _same_structure(g.norm_adj, norm)
    eq_bits(_np(g.norm_adj.val), np.asarray(vals, np.float32), "norm_adj")
    eq(_np(g.interaction_mat.val), _same_structure(g.interaction_mat, R))
    v = _same_structure(g.norm_interaction_mat, normR)
    eq_bits(_np(g.norm_interaction_mat.val), np.asarray(v, np.float32), "norm_interaction_mat")
    t = _canon(adj.T.tocsr())
    eq(_np(g.ui_adj.csc.rowptr), t.indptr)
    eq(_np(g.ui_adj.csc.col), t.indices)
    if case == "one_pair_5000_times":
        assert g.interaction_mat.nnz == 1 and _np(g.interaction_mat.val).tolist() == [5000.0]
