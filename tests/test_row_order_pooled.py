"""The pooled greedy row order on the host (hgd_row_order_greedy_pooled and
hgd_col_block_order_greedy_pooled, csrc/row_order_greedy.cpp): the XCDs of a group take their rows
in turn from one shared pool. Permutations and the layout at every shape and pool width, a pool of
one XCD pinned to hgd_row_order_greedy, the same order whatever the thread count, the refusals, the
modelled share of L2 hits against the order of parts walked alone (scripts/model_l2_order.py is the
judge), the environment switch, and the stand-alone sanitizer builds. No GPU."""
import functools
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from hypergraph_diffusion_for_recommendation_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 15, 16, 17, 8 * 16 * 3 - 1, 8 * 16 * 3 + 5]
POOLS = [1, 2, 4, 8]
C = 61
CAP = 4


@functools.lru_cache(maxsize=None)
def _model():
    spec = importlib.util.spec_from_file_location(
        "model_l2_order", os.path.join(ROOT, "scripts", "model_l2_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _graph(n_rows, seed, empty=True, n_cols=C, long_row=None):
    """(rowptr, col): rows of 0..12 ascending columns, every 7th row empty, column 0 in every third
    row (over CAP entries in any pool of 389 rows), and ``long_row`` holding every column."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n_rows):
        k = 0 if (empty and r % 7 == 3) else int(rng.integers(0 if empty else 1, 13))
        c = set(rng.choice(n_cols, size=k, replace=False).tolist())
        if k and r % 3 == 0:
            c.add(0)
        if r == long_row:
            c = set(range(n_cols))
        rows.append(np.array(sorted(c), dtype=np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    col = np.concatenate(rows + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return rowptr, col


def _args(rowptr, col):
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    return rowptr, col, col.ctypes.data if len(col) else None


def greedy(rowptr, col, n_cols, window=64, cap=CAP, R=16, xcds=8, chunks=1, threads=1):
    n = len(rowptr) - 1
    out = np.full(n + 1, -7, dtype=np.int32)  # (one past the end: never written)
    rowptr, col, cp = _args(rowptr, col)
    nat.check(nat.load().hgd_row_order_greedy(
        rowptr.ctypes.data, cp, n, n_cols, window, cap, R, xcds, chunks, threads,
        out.ctypes.data), "hgd_row_order_greedy")
    assert out[n] == -7
    return out[:n]


def pooled(rowptr, col, n_cols, pool, window=64, cap=CAP, R=16, xcds=8, threads=1):
    n = len(rowptr) - 1
    out = np.full(n + 1, -7, dtype=np.int32)
    rowptr, col, cp = _args(rowptr, col)
    nat.check(nat.load().hgd_row_order_greedy_pooled(
        rowptr.ctypes.data, cp, n, n_cols, window, cap, R, xcds, pool, threads,
        out.ctypes.data), "hgd_row_order_greedy_pooled")
    assert out[n] == -7
    return out[:n]


def greedy_blocks(rowptr, col, n_cols, P, window=64, cap=CAP, R=16, xcds=8, chunks=1, threads=1):
    n = len(rowptr) - 1
    out = np.full(n * P + 1, -7, dtype=np.int32)
    rowptr, col, cp = _args(rowptr, col)
    nat.check(nat.load().hgd_col_block_order_greedy(
        rowptr.ctypes.data, cp, n, n_cols, P, window, cap, R, xcds, chunks, threads,
        out.ctypes.data), "hgd_col_block_order_greedy")
    assert out[n * P] == -7
    return out[:n * P].reshape(P, n)


def pooled_blocks(rowptr, col, n_cols, P, pool, window=64, cap=CAP, R=16, xcds=8, threads=1):
    n = len(rowptr) - 1
    out = np.full(n * P + 1, -7, dtype=np.int32)
    rowptr, col, cp = _args(rowptr, col)
    nat.check(nat.load().hgd_col_block_order_greedy_pooled(
        rowptr.ctypes.data, cp, n, n_cols, P, window, cap, R, xcds, pool, threads,
        out.ctypes.data), "hgd_col_block_order_greedy_pooled")
    assert out[n * P] == -7
    return out[:n * P].reshape(P, n)


def _is_permutation(order, n):
    return order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(n))


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("R", [8, 16, 32])
@pytest.mark.parametrize("n_rows", SIZES)
def test_the_order_is_a_permutation_with_empty_rows_last(n_rows, R, pool):
    rowptr, col = _graph(n_rows, n_rows + 1)
    lens = np.diff(rowptr)
    if n_rows == SIZES[-1]:
        assert (col == 0).sum() > 8 * CAP  # column 0 is over the cap in every pool
    order = pooled(rowptr, col, C, pool, R=R)
    assert _is_permutation(order, n_rows)
    n_empty = int((lens == 0).sum())
    np.testing.assert_array_equal(order[n_rows - n_empty:], np.flatnonzero(lens == 0))


@pytest.mark.parametrize("pool", POOLS)
def test_all_rows_empty_a_row_longer_than_the_window_and_a_column_over_the_cap(pool):
    n = 8 * 16 * 3 + 5
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.testing.assert_array_equal(pooled(rowptr, np.zeros(0, np.int32), C, pool), np.arange(n))
    # row 40 holds all 61 columns: longer than a window of 16 gathers
    rowptr, col = _graph(n, 5, long_row=40)
    assert rowptr[41] - rowptr[40] == C > 16
    first = pooled(rowptr, col, C, pool, window=16)
    assert _is_permutation(first, n)
    np.testing.assert_array_equal(pooled(rowptr, col, C, pool, window=16, threads=5), first)
    # every column over the cap: no row is ever moved, the pool is walked in min-column order
    order = pooled(rowptr, col, C, pool, cap=1)
    assert _is_permutation(order, n)


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("R", [8, 16, 32])
@pytest.mark.parametrize("last_xcd", range(8))
def test_part_sizes_are_the_existing_builders(R, last_xcd, pool):
    """Workgroup w = positions [w·R, (w+1)·R) runs on XCD w mod 8 and only the last one is short.
    XCD x's sequence (position (8s + x)·R + j is its element s·R + j) has as many rows as the
    existing builder's part x, with the short last workgroup on every XCD in turn, and the XCDs of
    a pool hold between them exactly the natural range their parts cover."""
    n_wg = 8 * 2 + last_xcd + 1
    n = (n_wg - 1) * R + 5
    rowptr, col = _graph(n, 100 + n, empty=False)
    assert (np.diff(rowptr) > 0).all()
    order = pooled(rowptr, col, C, pool, R=R)
    old = greedy(rowptr, col, C, R=R)
    assert _is_permutation(order, n)
    seqs, off, bounds = [], 0, [0]
    for x in range(8):
        wgs = [w for w in range(n_wg) if w % 8 == x]
        size = sum(min(R, n - w * R) for w in wgs)
        assert size == len(wgs) * R - ((R - 5) if x == last_xcd else 0)
        pos = [(8 * s + x) * R + j for s, j in (divmod(t, R) for t in range(size))]
        seqs.append(order[pos])
        # the existing builder's part x is the natural range [off, off + size)
        np.testing.assert_array_equal(np.sort(old[pos]), np.arange(off, off + size))
        off += size
        bounds.append(off)
    assert off == n
    for q in range(8 // pool):
        got = np.sort(np.concatenate(seqs[q * pool:(q + 1) * pool]))
        np.testing.assert_array_equal(got, np.arange(bounds[q * pool], bounds[(q + 1) * pool]))


@pytest.mark.parametrize("R", [8, 16, 32])
@pytest.mark.parametrize("n_rows", SIZES)
def test_a_pool_of_one_xcd_is_the_existing_order(n_rows, R):
    rowptr, col = _graph(n_rows, n_rows + 1)
    np.testing.assert_array_equal(pooled(rowptr, col, C, 1, R=R), greedy(rowptr, col, C, R=R))


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("n_rows", [17, 129, 8 * 16 * 3 + 5])
def test_block_form(n_rows, P):
    """A pool of one XCD is hgd_col_block_order_greedy block for block; at every width every block
    is a permutation with the rows absent from the block last, and walked as a structure of its
    own is (a block is a pool of its own kind)."""
    rowptr, col = _graph(n_rows, 7 * n_rows + P)
    np.testing.assert_array_equal(pooled_blocks(rowptr, col, C, P, 1),
                                  greedy_blocks(rowptr, col, C, P))
    for pool in POOLS[1:]:
        got = pooled_blocks(rowptr, col, C, P, pool)
        for threads in (2, 3, 8, 16):
            np.testing.assert_array_equal(
                pooled_blocks(rowptr, col, C, P, pool, threads=threads), got)
        for k in range(P):
            lo, hi = C * k // P, C * (k + 1) // P  # hgd_spmm_col_blocks' cuts
            assert _is_permutation(got[k], n_rows)
            pieces = [col[rowptr[r]:rowptr[r + 1]] for r in range(n_rows)]
            pieces = [p[(p >= lo) & (p < hi)] - lo for p in pieces]
            bptr = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)
            bcol = np.concatenate(pieces + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
            absent = np.flatnonzero(np.diff(bptr) == 0)
            np.testing.assert_array_equal(got[k][n_rows - len(absent):], absent)
            np.testing.assert_array_equal(got[k], pooled(bptr, bcol, hi - lo, pool))


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("n_rows", [17, 8 * 16 * 3 - 1, 8 * 16 * 3 + 5])
def test_the_order_does_not_depend_on_the_thread_count(n_rows, pool):
    rowptr, col = _graph(n_rows, n_rows + 1)
    first = pooled(rowptr, col, C, pool, threads=1)
    for threads in (2, 3, 8, 16):
        np.testing.assert_array_equal(pooled(rowptr, col, C, pool, threads=threads), first)


@pytest.mark.parametrize("pool", POOLS[1:])
def test_a_long_window_takes_several_rows_a_round(pool):
    """Where 1/128 of the window holds several rows, a walker takes up to 8 rows a round: 2,005
    rows under a window that never fills (so one of all the pool's gathers) make rounds of 3, 6
    and 8 rows at pools of 2, 4 and 8 XCDs, the last round short."""
    n = 2005
    rowptr, col = _graph(n, 77)
    lens = np.diff(rowptr)
    m = int((lens > 0).sum())
    assert min(8, m * pool // 8 // 128) == {2: 3, 4: 6, 8: 8}[pool]
    first = pooled(rowptr, col, C, pool, window=1 << 20)
    assert _is_permutation(first, n)
    np.testing.assert_array_equal(first[m:], np.flatnonzero(lens == 0))
    for threads in (2, 3, 16):
        np.testing.assert_array_equal(
            pooled(rowptr, col, C, pool, window=1 << 20, threads=threads), first)
    # every pool's XCDs hold the natural range of their parts between them
    xcd = (np.arange(m) // 16) % 8
    off = 0
    for q in range(8 // pool):
        got = np.sort(first[:m][(xcd // pool) == q])
        np.testing.assert_array_equal(got, np.flatnonzero(lens > 0)[off:off + len(got)])
        off += len(got)
    assert off == m


def test_bad_arguments_are_refused():
    lib = nat.load()
    rowptr = np.array([0, 2], dtype=np.int64)
    col = np.array([1, 99], dtype=np.int32)
    out = np.zeros(2, dtype=np.int32)

    def row(window=64, cap=16, R=16, xcds=8, pool=8, threads=1, n_cols=10):
        return lib.hgd_row_order_greedy_pooled(rowptr.ctypes.data, col.ctypes.data, 1, n_cols,
                                               window, cap, R, xcds, pool, threads,
                                               out.ctypes.data)

    def blk(ptr=col, n_blocks=2, xcds=8, pool=8):
        return lib.hgd_col_block_order_greedy_pooled(rowptr.ctypes.data, ptr.ctypes.data, 1, 10,
                                                     n_blocks, 64, 16, 16, xcds, pool, 1,
                                                     out.ctypes.data)

    assert row(n_cols=100) == 0
    # (no arguments: column 99 of 10; pool=0 stands where chunks=0 stood)
    for bad in (dict(), dict(window=0), dict(cap=0), dict(R=0), dict(xcds=0), dict(pool=0),
                dict(threads=-1), dict(pool=3, n_cols=100), dict(pool=16, n_cols=100),
                dict(xcds=6, pool=4, n_cols=100)):
        assert row(**bad) == 1, bad  # HGD_ERR_INVALID_ARG
        assert "hgd_row_order_greedy_pooled" in lib.hgd_get_last_error_string().decode()
    assert row(xcds=6, pool=3, n_cols=100) == 0
    desc = np.array([5, 1], dtype=np.int32)
    assert blk(ptr=desc) == 1
    assert "do not ascend" in lib.hgd_get_last_error_string().decode()
    assert "hgd_col_block_order_greedy_pooled" in lib.hgd_get_last_error_string().decode()
    # a column out of range is an invalid argument in both forms, and says so
    assert row() == 1
    assert "a column outside [0, n_cols)" in lib.hgd_get_last_error_string().decode()
    assert "memory" not in lib.hgd_get_last_error_string().decode()
    for bad in (dict(), dict(n_blocks=65, ptr=desc), dict(pool=3), dict(pool=0)):
        assert blk(**bad) == 1, bad
        assert "hgd_col_block_order_greedy_pooled" in lib.hgd_get_last_error_string().decode()


@functools.lru_cache(maxsize=None)
def _model_graph():
    """50,000 × 5,000 × 500,000 draws, seed 0 (scale 0.005 of the bench graph; window 81)."""
    m = _model()
    rowptr, col = m.make_graph(50_000, 5_000, 500_000, 0)
    return rowptr.astype(np.int64), col.astype(np.int32)


def test_hit_share_into_users_of_one_pool_of_eight():
    """One pool of all 8 XCDs against 8 parts walked alone. The issue's model: 21.59 % -> 27.55 %
    for one sequence cut in 8, 20.29 % -> 25.96 % for a crude shared-pool stand-in; the bound is
    the issue's, 0.04 above the existing placed order."""
    m = _model()
    rowptr, col = _model_graph()
    U, I, window = 50_000, 5_000, 81
    old = greedy(rowptr, col, I, window=window, cap=1024, R=m.ROWS_PER_WG, xcds=m.XCDS, chunks=1,
                 threads=0)
    new = pooled(rowptr, col, I, 8, window=window, cap=1024, R=m.ROWS_PER_WG, xcds=m.XCDS,
                 threads=0)
    assert _is_permutation(new, U)
    before, got = m.hit_share(rowptr, col, old, window), m.hit_share(rowptr, col, new, window)
    print(f"into users: parts walked alone {100 * before:.2f} %, one pool of 8 {100 * got:.2f} %")
    assert got >= before + 0.04


def test_hit_share_of_a_block_into_items_of_one_pool_of_eight():
    """Block 0 of 4 of the transposed graph. The issue's model: 6.74 % -> 9.16 %; the bound is the
    issue's, 0.015 above the existing order."""
    m = _model()
    rowptr, col = _model_graph()
    U, I, window, P = 50_000, 5_000, 81, 4
    cptr, crow = m.transpose(rowptr, col, I)
    cut = U // P
    keep = crow < cut
    bptr = np.concatenate([[0], np.cumsum(keep)])[cptr]
    bcol = crow[keep]
    cptr, crow = cptr.astype(np.int64), crow.astype(np.int32)
    old = greedy_blocks(cptr, crow, U, P, window=window, cap=1024, R=m.ROWS_PER_WG, xcds=m.XCDS,
                        chunks=1, threads=0)[0]
    new = pooled_blocks(cptr, crow, U, P, 8, window=window, cap=1024, R=m.ROWS_PER_WG,
                        xcds=m.XCDS, threads=0)[0]
    assert _is_permutation(new, I)
    before, got = m.hit_share(bptr, bcol, old, window), m.hit_share(bptr, bcol, new, window)
    print(f"into items, block 0 of {P}: parts walked alone {100 * before:.2f} %, one pool of 8 "
          f"{100 * got:.2f} %")
    assert got >= before + 0.015


def test_pool_environment_switch(monkeypatch):
    from hypergraph_diffusion_for_recommendation_amd import incidence
    from hypergraph_diffusion_for_recommendation_amd.incidence import (order_geometry,
                                                                      order_pool_width)
    monkeypatch.delenv("HGD_SPMM_ORDER_POOL", raising=False)
    monkeypatch.delenv("HGD_SPMM_ORDER_PLACE", raising=False)
    assert order_pool_width() == incidence.ORDER_XCDS_PER_POOL
    assert incidence.ORDER_XCDS_PER_POOL in (1, 2, 4, 8)
    geom = order_geometry(64, False), order_geometry(64, True)
    assert geom[0] == (16384, 16, 8, 1)
    for good in ("1", "2", "4", "8"):
        monkeypatch.setenv("HGD_SPMM_ORDER_POOL", good)
        assert order_pool_width() == int(good)
        # neither the geometry nor the key the orders are cached under knows of it
        assert (order_geometry(64, False), order_geometry(64, True)) == geom
    for bad in ("0", "3", "16", " 8", "8 ", "08", "auto", "-1"):
        monkeypatch.setenv("HGD_SPMM_ORDER_POOL", bad)
        with pytest.raises(ValueError, match="HGD_SPMM_ORDER_POOL"):
            order_pool_width()


def test_csr_takes_the_pooled_order_under_the_unchanged_key(monkeypatch):
    """CSR._greedy_order on the CPU: the pooled builders at the width the switch says, the parent's
    order at 1 and with HGD_SPMM_ORDER_PLACE=0, cached under (P, window, R, 8, 1)."""
    import torch
    from hypergraph_diffusion_for_recommendation_amd.incidence import CSR
    monkeypatch.delenv("HGD_SPMM_ORDER_POOL", raising=False)
    n = 8 * 16 * 3 + 5
    rowptr, col = _graph(n, 11)
    geom = (64, 16, 8, 1)

    def csr():
        return CSR(torch.from_numpy(rowptr), torch.from_numpy(col), n, C, split_threshold=0)

    from hypergraph_diffusion_for_recommendation_amd import incidence
    want = pooled(rowptr, col, C, incidence.ORDER_XCDS_PER_POOL, cap=nat.ORDER_COL_CAP, threads=0)
    np.testing.assert_array_equal(csr()._greedy_order(0, geom).numpy(), want)
    for width in (1, 2, 4, 8):
        monkeypatch.setenv("HGD_SPMM_ORDER_POOL", str(width))
        np.testing.assert_array_equal(
            csr()._greedy_order(0, geom).numpy(),
            pooled(rowptr, col, C, width, cap=nat.ORDER_COL_CAP))
        np.testing.assert_array_equal(
            csr()._greedy_order(3, geom).numpy().reshape(3, n),
            pooled_blocks(rowptr, col, C, 3, width, cap=nat.ORDER_COL_CAP))
    monkeypatch.setenv("HGD_SPMM_ORDER_POOL", "1")
    np.testing.assert_array_equal(csr()._greedy_order(0, geom).numpy(),
                                  greedy(rowptr, col, C, cap=nat.ORDER_COL_CAP))
    monkeypatch.setenv("HGD_SPMM_ORDER_POOL", "8")
    # unplaced (HGD_SPMM_ORDER_PLACE=0's geometry): the old builder, whatever the width
    np.testing.assert_array_equal(
        csr()._greedy_order(0, (64, 16, 1, 8)).numpy(),
        greedy(rowptr, col, C, cap=nat.ORDER_COL_CAP, xcds=1, chunks=8))


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_stand_alone_program_runs_clean_under_sanitizers(tmp_path, sanitizers):
    """csrc/row_order_greedy.cpp with tests/native/row_order_pooled_main.cpp (its own main; not
    loaded into Python): every pool width with 1 to 16 threads."""
    # the sanitizer's runtime linked into the program itself (clang's default, g++'s -static-lib*):
    # it does not depend on the order the dynamic loader brings libraries in
    gxx = shutil.which("g++")
    clang = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if gxx is not None:
        cmd = [gxx] + [f"-static-lib{s}" for s in
                       {"address,undefined": ("asan", "ubsan"), "thread": ("tsan",)}[sanitizers]]
    elif os.path.exists(clang):
        cmd = [clang]
    else:
        pytest.fail("no host C++ compiler (g++ / clang++) to build the stand-alone program with")
    exe = str(tmp_path / "row_order_pooled")
    src = [os.path.join(ROOT, "hypergraph_diffusion_for_recommendation_amd", "csrc",
                        "row_order_greedy.cpp"),
           os.path.join(ROOT, "tests", "native", "row_order_pooled_main.cpp")]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={sanitizers}",
                          "-fno-sanitize-recover=all", "-o", exe] + src, check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout
    assert "all orders are permutations" in run.stdout
    assert "Sanitizer" not in run.stdout and "runtime error" not in run.stdout
