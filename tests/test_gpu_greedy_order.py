"""GPU: the ordered hops over the greedy shared-column order (hgd_row_order_greedy /
hgd_col_block_order_greedy on the host, hgd_spmm_row_order_from /
hgd_spmm_col_blocks_ordered_from on the device) are bit for bit the hops in natural order; the
builders split into a sort and a tail reproduce the min-column arrays; a non-permutation is
refused before anything is read through it."""
import functools

import numpy as np
import pytest
import torch

from tests._util import random_coo

pytestmark = pytest.mark.gpu

C = 129
# (n_rows = 0 has no hop to compare: spmm_csr never orders a structure without nonzeros. The
# entry points themselves take it: test_from_builders_reproduce_the_min_column_arrays calls the
# _from builders and hgd_spmm_ordered with no rows.)
SIZES = [1, 15, 16, 17, 127, 128, 129, 8 * 16 * 3 + 5]
WINDOW = 64  # far below the structures' nonzeros: columns leave the window again
HGD_ERR_INVALID_ARG = 1


@functools.lru_cache(maxsize=None)
def _case(R, n_cols=C):
    """An Incidence of R rows over n_cols columns, ~10 nonzeros a row, with empty rows, weighted."""
    from hypergraph_diffusion_for_recommendation_amd import Incidence
    rng = np.random.default_rng(500 + R)
    r, c = random_coo(rng, R, n_cols, 10 * R)
    keep = ~np.isin(r, [3, 50, 51, R - 1]) if R > 100 else np.ones(len(r), dtype=bool)
    r, c = r[keep], c[keep]
    vals = rng.standard_normal(len(r)).astype(np.float32)
    return Incidence.from_coo(torch.from_numpy(np.stack([r, c])), torch.from_numpy(vals),
                              (R, n_cols), device="cuda:0", rows_sorted=True,
                              split_threshold=0).persist()


@pytest.fixture
def small_window(monkeypatch):
    """The greedy order with a window of 64 gathers and the hop's own rows per workgroup."""
    from hypergraph_diffusion_for_recommendation_amd import incidence
    real = incidence.order_geometry
    monkeypatch.setattr(incidence, "order_geometry",
                        lambda d, blocked: (WINDOW,) + real(d, blocked)[1:])
    monkeypatch.setenv("HGD_SPMM_ORDER_KIND", "2")
    for name in ("HGD_SPMM_ORDER_PLACE", "HGD_SPMM_PACKED", "HGD_SPMM_BLOCKS"):
        monkeypatch.delenv(name, raising=False)
    return real


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("R", SIZES)
def test_ordered_hop_under_the_greedy_order_is_bitwise_the_plain_hop(dev, monkeypatch,
                                                                     small_window, R, d):
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    inc = _case(R)
    csr = inc.csr
    rng = np.random.default_rng(d * 31 + R)
    X = torch.from_numpy(rng.standard_normal((C, d)).astype(np.float32)).to(dev)
    q = torch.from_numpy(rng.standard_normal(R).astype(np.float32)).to(dev)
    kw = dict(val=inc.val, row_scale=q, epilogue=nat.EPI_LEAKY_RELU, slope=0.2)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "0")
    plain = spmm_csr(csr, X, **kw)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "1")
    Y = torch.full((R, d), float("nan"), device=dev)
    spmm_csr(csr, X, out=Y, **kw)
    assert torch.equal(Y, plain)
    # the greedy order was the one walked: built once per geometry, a permutation with the empty
    # rows last, and not the min-column order
    rows_per_wg = small_window(d, False)[1]
    assert rows_per_wg == {32: 32, 64: 16, 128: 8}[d]
    key = (0, WINDOW, rows_per_wg, 8, 1)
    assert key in csr._greedy
    order = csr._greedy[key][0].cpu().numpy()
    np.testing.assert_array_equal(np.sort(order), np.arange(R))
    lens = (csr.rowptr[1:] - csr.rowptr[:-1]).cpu().numpy()
    n_empty = int((lens == 0).sum())
    np.testing.assert_array_equal(order[R - n_empty:], np.flatnonzero(lens == 0))
    from hypergraph_diffusion_for_recommendation_amd.incidence import order_geometry
    geom = order_geometry(d, False)  # (the fixture's: window 64)
    assert (0,) + geom == key
    assert csr.row_order(nat.ORDER_GREEDY, geom) is csr.row_order(nat.ORDER_GREEDY, geom)
    assert csr.row_order(nat.ORDER_GREEDY, geom) is csr._greedy[key]
    if R > 100:
        assert not np.array_equal(order, csr.row_order()[0].cpu().numpy())


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("R,d", [(17, 64), (129, 32), (8 * 16 * 3 + 5, 64), (8 * 16 * 3 + 5, 128)])
def test_blocked_hops_under_the_greedy_block_orders_are_bitwise_the_blocked_hop(
        dev, monkeypatch, small_window, R, d, P):
    """The CSC of a binary incidence with a degree scale as its weights, so the same hop runs as
    hgd_spmm_blocked, hgd_spmm_blocked_ordered and hgd_spmm_blocked_packed."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    csc = _case(R).csc  # C rows over R columns; its rows' columns ascend
    assert csc.cols_ascending and csc.n_rows == C and csc.n_cols == R
    rng = np.random.default_rng(d + 7 * R + P)
    X = torch.from_numpy(rng.standard_normal((R, d)).astype(np.float32)).to(dev)
    q = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(dev)
    src = torch.from_numpy(rng.integers(1, 9, R).astype(np.float32) ** -0.5).to(dev)
    val = src[csc.col.long()]
    kw = dict(val=val, row_scale=q, epilogue=nat.EPI_LEAKY_RELU, slope=0.2, src_scale=src)
    monkeypatch.setenv("HGD_SPMM_BLOCKS", str(P))
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "0")
    blocked = spmm_csr(csc, X, **kw)
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "1")
    monkeypatch.setenv("HGD_SPMM_PACKED", "0")
    ordered = spmm_csr(csc, X, out=torch.full((C, d), float("nan"), device=dev), **kw)
    monkeypatch.setenv("HGD_SPMM_PACKED", "1")
    packed = spmm_csr(csc, X, out=torch.full((C, d), float("nan"), device=dev), **kw)
    assert torch.equal(ordered, blocked)
    assert torch.equal(packed, blocked)
    key = (P, WINDOW, small_window(d, True)[1], 8, 1)
    assert key in csc._greedy
    assert any(k[0] == key for k in csc._packed)  # the packed entries of this order
    start, _, _, out_row = (t.cpu().numpy() for t in csc._greedy[key])
    lens = np.diff(start)
    for k in range(P):
        rows = out_row[k * C:(k + 1) * C]
        np.testing.assert_array_equal(np.sort(rows), np.arange(C))
        piece = lens[k * C:(k + 1) * C]  # rows without a nonzero in the block last
        assert (piece[:int((piece > 0).sum())] > 0).all()


def test_from_builders_reproduce_the_min_column_arrays(dev):
    """hgd_spmm_row_order and hgd_spmm_col_blocks_ordered are a sort and the tail the _from entry
    points run: over the min-column orders those return the same arrays bit for bit."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import _stream, _ws
    R, P = 8 * 16 * 3 + 5, 3
    inc = _case(R)
    lib, st = nat.load(), _stream(dev)
    csr = inc.csr
    order, rowptr_o, col_o, perm = csr.row_order()
    got = (torch.full_like(rowptr_o, -1), torch.full_like(col_o, -1), torch.full_like(perm, -1))
    ws = _ws(lib.hgd_spmm_row_order_from_workspace_size(R), dev)
    nat.check(lib.hgd_spmm_row_order_from(
        order.data_ptr(), csr.rowptr.data_ptr(), csr.col.data_ptr(), R, C, got[0].data_ptr(),
        got[1].data_ptr(), got[2].data_ptr(), ws.data_ptr(), ws.numel(), st), "row_order_from")
    for a, b in zip(got, (rowptr_o, col_o, perm)):
        assert torch.equal(a, b)
    csc = inc.csc
    start, bcol, bperm, out_row = csc.col_blocks_ordered(P)
    got = (torch.full_like(start, -1), torch.full_like(bcol, -1), torch.full_like(bperm, -1))
    ws = _ws(lib.hgd_spmm_col_blocks_ordered_from_workspace_size(C, P), dev)
    nat.check(lib.hgd_spmm_col_blocks_ordered_from(
        out_row.data_ptr(), csc.rowptr.data_ptr(), csc.col.data_ptr(), C, R, P, got[0].data_ptr(),
        got[1].data_ptr(), got[2].data_ptr(), ws.data_ptr(), ws.numel(), st), "col_blocks_from")
    for a, b in zip(got, (start, bcol, bperm)):
        assert torch.equal(a, b)
    # an empty structure is nothing to do; a short workspace is refused
    assert lib.hgd_spmm_row_order_from(None, None, None, 0, C, None, None, None, None, 0, st) == 0
    assert lib.hgd_spmm_col_blocks_ordered_from(None, None, None, 0, R, P, None, None, None, None,
                                                0, st) == 0
    assert lib.hgd_spmm_row_order_from(
        order.data_ptr(), csr.rowptr.data_ptr(), csr.col.data_ptr(), R, C, got[0].data_ptr(),
        got[1].data_ptr(), got[2].data_ptr(), ws.data_ptr(), 16, st) == 4  # HGD_ERR_WORKSPACE
    # ... and so is the ordered hop over no rows
    X = torch.zeros(C, 64, device=dev)
    assert lib.hgd_spmm_ordered(None, None, None, None, 0, C, 0, 0, X.data_ptr(), 64, None, 64, 64,
                                0, 0.0, None, None, 0, None, st) == 0


def test_a_non_permutation_is_refused(dev):
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import _stream, _ws
    R, P = 129, 3
    inc = _case(R)
    lib, st = nat.load(), _stream(dev)
    csr, csc = inc.csr, inc.csc
    good = torch.randperm(R, device=dev).to(torch.int32)
    out = (torch.full((R + 1,), -1, dtype=torch.int64, device=dev),
           torch.full((csr.nnz,), -1, dtype=torch.int32, device=dev),
           torch.full((csr.nnz,), -1, dtype=torch.int32, device=dev))
    ws = _ws(lib.hgd_spmm_row_order_from_workspace_size(R), dev)

    def row(order):
        return lib.hgd_spmm_row_order_from(
            order.data_ptr(), csr.rowptr.data_ptr(), csr.col.data_ptr(), R, C, out[0].data_ptr(),
            out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(), st)

    for what, at, value in (("twice", 5, int(good[6])), ("past the end", 0, R),
                            ("far past the end", R - 1, 2 ** 31 - 1), ("negative", 7, -1)):
        bad = good.clone()
        bad[at] = value
        assert row(bad) == HGD_ERR_INVALID_ARG, what
        assert "not a permutation" in lib.hgd_get_last_error_string().decode()
    torch.cuda.synchronize()
    assert all(bool((t == -1).all()) for t in out)  # nothing was built through a bad order
    assert row(good) == 0

    goods = torch.cat([torch.randperm(C, device=dev) for _ in range(P)]).to(torch.int32)
    outb = (torch.full((P * C + 1,), -1, dtype=torch.int64, device=dev),
            torch.full((csc.nnz,), -1, dtype=torch.int32, device=dev),
            torch.full((csc.nnz,), -1, dtype=torch.int32, device=dev))
    wsb = _ws(lib.hgd_spmm_col_blocks_ordered_from_workspace_size(C, P), dev)

    def blocks(order):
        return lib.hgd_spmm_col_blocks_ordered_from(
            order.data_ptr(), csc.rowptr.data_ptr(), csc.col.data_ptr(), C, R, P,
            outb[0].data_ptr(), outb[1].data_ptr(), outb[2].data_ptr(), wsb.data_ptr(),
            wsb.numel(), st)

    # a permutation of all P·C positions that is none per block: block 0 names a row twice and
    # block 1 makes up for it
    bad = goods.clone()
    twice = int(bad[0])
    bad[1], bad[C + int((goods[C:2 * C] == twice).nonzero())] = twice, int(goods[1])
    assert int(bad.sum()) == int(goods.sum())
    assert blocks(bad) == HGD_ERR_INVALID_ARG
    assert "hgd_spmm_col_blocks_ordered_from" in lib.hgd_get_last_error_string().decode()
    bad = goods.clone()
    bad[2 * C + 3] = C
    assert blocks(bad) == HGD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert all(bool((t == -1).all()) for t in outb)
    assert blocks(goods) == 0


def test_hgconv2_backward_equals_its_forward_under_the_greedy_orders(dev, monkeypatch,
                                                                     small_window):
    """The normalised two-hop is a symmetric operator: the gradient for W is the forward of W,
    through the same two hops, under the greedy orders as without any."""
    from hypergraph_diffusion_for_recommendation_amd import Incidence, hgconv2
    rng = np.random.default_rng(9)
    U, I, d = 1000, 300, 64
    r, c = random_coo(rng, U, I, 9000)
    X = torch.from_numpy(rng.standard_normal((U, d)).astype(np.float32)).to(dev)
    W = torch.from_numpy(rng.standard_normal((U, d)).astype(np.float32)).to(dev)
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    got = {}
    for env in ("0", "1"):
        inc = Incidence.from_coo(torch.from_numpy(np.stack([r, c])), None, (U, I), device=dev,
                                 split_threshold=0).persist()
        monkeypatch.setenv("HGD_SPMM_ROW_ORDER", env)
        monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", env)
        Xr = X.clone().requires_grad_(True)
        Y = hgconv2(inc, Xr)
        (dX,) = torch.autograd.grad(Y, Xr, W)
        got[env] = (Y.detach(), dX, hgconv2(inc, W))
        greedy = {k[0] for s in (inc.csr, inc.csc) for k in s._greedy}
        # (0: the hop into users' row order; 3: the three blocks' orders of a blocked hop)
        assert (3 in greedy and greedy <= {0, 3}) if env == "1" else not greedy
    for a, b in zip(got["1"], got["0"]):
        assert torch.equal(a, b)
    assert torch.equal(got["1"][1], got["1"][2])  # backward of W == forward of W


def test_a_dropped_structure_over_the_size_rule_never_builds_a_greedy_order(dev, monkeypatch):
    """Incidence.drop makes new structures on every training step, possibly inside a captured
    step: over the size rule (a 32 MiB table, short rows) their hop is ordered, but in min-column
    order, built on the stream without a host synchronisation — while the persistent parent's
    same hop builds the greedy order. Not even HGD_SPMM_ORDER_KIND=2 changes that."""
    from hypergraph_diffusion_for_recommendation_amd import Incidence, spmm_csr
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import (spmm_order_kind,
                                                                      spmm_row_order)
    for name in ("HGD_SPMM_ROW_ORDER", "HGD_SPMM_ORDER_KIND", "HGD_SPMM_ORDER_PLACE"):
        monkeypatch.delenv(name, raising=False)
    U, I, d = 40_000, 131_072, 64  # the table: 131,072 rows of 256 B = 32 MiB
    rng = np.random.default_rng(3)
    r, c = random_coo(rng, U, I, 10 * U)
    parent = Incidence.from_coo(torch.from_numpy(np.stack([r, c])), None, (U, I), device=dev,
                                rows_sorted=True)
    X = torch.from_numpy(rng.standard_normal((I, d)).astype(np.float32)).to(dev)
    mask = torch.from_numpy(rng.random(parent.nnz) < 0.5).to(dev)
    for capacity in (False, True):
        child = parent.drop(mask, 0.5, capacity=capacity)
        assert not child.csr.persistent and not child.csc.persistent
        assert spmm_row_order(child.csr, d)  # the size rule orders its hop ...
        for env in (None, "2"):
            if env:
                monkeypatch.setenv("HGD_SPMM_ORDER_KIND", env)
            assert spmm_order_kind(child.csr, d) == nat.ORDER_MIN_COLUMN  # ... by min column
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")  # a host synchronisation raises
            try:
                Y = spmm_csr(child.csr, X)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert not child.csr._greedy and child.csr._row_order is not None
        monkeypatch.delenv("HGD_SPMM_ORDER_KIND")
        monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "0")
        assert torch.equal(Y, spmm_csr(child.csr, X))
        monkeypatch.delenv("HGD_SPMM_ROW_ORDER")
    # the parent: min column until it is said to persist, greedy after
    assert spmm_order_kind(parent.csr, d) == nat.ORDER_MIN_COLUMN
    parent.persist()
    assert spmm_order_kind(parent.csr, d) == nat.ORDER_GREEDY
    Y = spmm_csr(parent.csr, X)
    assert [k[0] for k in parent.csr._greedy] == [0] and parent.csr._row_order is None
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "0")
    assert torch.equal(Y, spmm_csr(parent.csr, X))
