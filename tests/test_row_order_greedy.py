"""The greedy shared-column row order on the host (hgd_row_order_greedy and
hgd_col_block_order_greedy, csrc/row_order_greedy.cpp): permutations at every shape, the same
order whatever the thread count, the XCD placement position by position, the per-block form, the
modelled share of L2 hits against the min-column order (scripts/model_l2_order.py is the judge),
and the stand-alone sanitizer builds. No GPU."""
import ctypes
import functools
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from hypergraph_diffusion_for_recommendation_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 15, 16, 17, 127, 128, 129, 8 * 16 * 3 + 5]
C = 61
CAP = 4


@functools.lru_cache(maxsize=None)
def _model():
    spec = importlib.util.spec_from_file_location(
        "model_l2_order", os.path.join(ROOT, "scripts", "model_l2_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _graph(n_rows, seed, empty=True, n_cols=C):
    """(rowptr, col): rows of 0..12 ascending columns, every 7th row empty, and column 0 in every
    third row: of 389 rows over 8 parts it has over CAP entries in every chunk."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n_rows):
        k = 0 if (empty and r % 7 == 3) else int(rng.integers(0 if empty else 1, 13))
        c = set(rng.choice(n_cols, size=k, replace=False).tolist())
        if k and r % 3 == 0:
            c.add(0)
        rows.append(np.array(sorted(c), dtype=np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    col = np.concatenate(rows + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return rowptr, col


def greedy(rowptr, col, n_cols, window=64, cap=CAP, R=16, xcds=8, chunks=1, threads=1):
    n = len(rowptr) - 1
    out = np.full(n + 1, -7, dtype=np.int32)  # (one past the end: never written)
    col = np.ascontiguousarray(col, dtype=np.int32)
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    nat.check(nat.load().hgd_row_order_greedy(
        rowptr.ctypes.data, col.ctypes.data if len(col) else None, n, n_cols, window, cap, R, xcds,
        chunks, threads, out.ctypes.data), "hgd_row_order_greedy")
    assert out[n] == -7
    return out[:n]


def greedy_blocks(rowptr, col, n_cols, P, window=64, cap=CAP, R=16, xcds=8, chunks=1, threads=1):
    n = len(rowptr) - 1
    out = np.full(n * P + 1, -7, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    nat.check(nat.load().hgd_col_block_order_greedy(
        rowptr.ctypes.data, col.ctypes.data if len(col) else None, n, n_cols, P, window, cap, R,
        xcds, chunks, threads, out.ctypes.data), "hgd_col_block_order_greedy")
    assert out[n * P] == -7
    return out[:n * P].reshape(P, n)


def _is_permutation(order, n):
    return order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(n))


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("R", [8, 16, 32])
@pytest.mark.parametrize("n_rows", SIZES)
def test_the_order_is_a_permutation_whatever_the_thread_count(n_rows, R, chunks):
    rowptr, col = _graph(n_rows, n_rows + 1)
    lens = np.diff(rowptr)
    if n_rows == SIZES[-1] and chunks == 1:
        # column 0 is over the cap in every chunk, and still every row is placed once
        assert min((col[rowptr[b]:rowptr[e]] == 0).sum()
                   for b, e in zip(range(0, 336, 48), range(48, 384, 48))) > CAP
    first = greedy(rowptr, col, C, R=R, chunks=chunks, threads=1)
    assert _is_permutation(first, n_rows)
    # empty rows last, in natural order
    n_empty = int((lens == 0).sum())
    np.testing.assert_array_equal(first[n_rows - n_empty:], np.flatnonzero(lens == 0))
    for threads in (2, 7):
        np.testing.assert_array_equal(
            greedy(rowptr, col, C, R=R, chunks=chunks, threads=threads), first)


def _sub(rowptr, col, rows):
    """The structure of the given rows alone."""
    lens = np.diff(rowptr)[rows]
    cols = [col[rowptr[r]:rowptr[r + 1]] for r in rows] + [np.zeros(0, dtype=np.int32)]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(cols)


@pytest.mark.parametrize("R", [8, 16, 32])
@pytest.mark.parametrize("last_xcd", range(8))
def test_placement_position_by_position(R, last_xcd):
    """Workgroup w = positions [w·R, (w+1)·R) runs on XCD w mod 8 and only the last one is short:
    part x is the natural range of as many rows as XCD x's workgroups hold, walked on its own, and
    position (8s + x)·R + j takes element s·R + j of part x — with the short last workgroup on
    every XCD in turn."""
    n_wg = 8 * 2 + last_xcd + 1
    n = (n_wg - 1) * R + 5
    rowptr, col = _graph(n, 100 + n, empty=False)
    assert (np.diff(rowptr) > 0).all()
    order = greedy(rowptr, col, C, R=R)
    assert _is_permutation(order, n)
    off = 0
    for x in range(8):
        wgs = [w for w in range(n_wg) if w % 8 == x]
        size = sum(min(R, n - w * R) for w in wgs)
        assert size == len(wgs) * R - ((R - 5) if x == last_xcd else 0)
        part = np.arange(off, off + size)
        # the part walked alone, as one sequence
        seq = part[greedy(*_sub(rowptr, col, part), C, R=R, xcds=1)]
        for t, row in enumerate(seq):
            s, j = divmod(t, R)
            assert order[(8 * s + x) * R + j] == row, (x, t)
        off += size
    assert off == n


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("n_rows", [17, 129, 8 * 16 * 3 + 5])
def test_block_form_orders_every_block_and_puts_absent_rows_last(n_rows, P):
    rowptr, col = _graph(n_rows, 7 * n_rows + P)
    got = greedy_blocks(rowptr, col, C, P, chunks=1)
    for threads in (2, 7):
        np.testing.assert_array_equal(greedy_blocks(rowptr, col, C, P, threads=threads), got)
    absent_somewhere = 0
    for k in range(P):
        lo, hi = C * k // P, C * (k + 1) // P  # hgd_spmm_col_blocks' cuts
        assert _is_permutation(got[k], n_rows)
        # block k's own structure, its columns counted from the block's first
        pieces = [col[rowptr[r]:rowptr[r + 1]] for r in range(n_rows)]
        pieces = [p[(p >= lo) & (p < hi)] - lo for p in pieces]
        bptr = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)
        bcol = np.concatenate(pieces + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
        absent = np.flatnonzero(np.diff(bptr) == 0)
        absent_somewhere += len(absent)
        np.testing.assert_array_equal(got[k][n_rows - len(absent):], absent)
        # ... is walked as a structure of its own is
        np.testing.assert_array_equal(got[k], greedy(bptr, bcol, hi - lo))
    assert absent_somewhere > n_rows // 7  # rows that miss a block beyond the empty ones


def test_bad_arguments_are_refused():
    lib = nat.load()
    rowptr = np.array([0, 2], dtype=np.int64)
    col = np.array([1, 99], dtype=np.int32)
    out = np.zeros(2, dtype=np.int32)

    def row(window=64, cap=16, R=16, xcds=8, chunks=1, threads=1, n_cols=10):
        return lib.hgd_row_order_greedy(rowptr.ctypes.data, col.ctypes.data, 1, n_cols, window, cap,
                                        R, xcds, chunks, threads, out.ctypes.data)

    assert row(n_cols=100) == 0
    for bad in (dict(), dict(window=0), dict(cap=0), dict(R=0), dict(xcds=0), dict(chunks=0),
                dict(threads=-1)):
        assert row(**bad) == 1, bad  # HGD_ERR_INVALID_ARG (no arguments: column 99 of 10)
        assert "hgd_row_order_greedy" in lib.hgd_get_last_error_string().decode()
    desc = np.array([5, 1], dtype=np.int32)
    assert lib.hgd_col_block_order_greedy(rowptr.ctypes.data, desc.ctypes.data, 1, 10, 2, 64, 16,
                                          16, 8, 1, 1, out.ctypes.data) == 1
    assert "do not ascend" in lib.hgd_get_last_error_string().decode()
    # a column out of range is an invalid argument in both forms, and says so
    assert row() == 1
    assert "a column outside [0, n_cols)" in lib.hgd_get_last_error_string().decode()
    assert "memory" not in lib.hgd_get_last_error_string().decode()
    assert lib.hgd_col_block_order_greedy(rowptr.ctypes.data, col.ctypes.data, 1, 10, 2, 64, 16,
                                          16, 8, 1, 1, out.ctypes.data) == 1
    assert lib.hgd_col_block_order_greedy(rowptr.ctypes.data, desc.ctypes.data, 1, 10, 65, 64, 16,
                                          16, 8, 1, 1, out.ctypes.data) == 1


@functools.lru_cache(maxsize=None)
def _model_graph():
    """50,000 × 5,000 × 500,000 draws, seed 0 (scale 0.005 of the bench graph; window 81)."""
    m = _model()
    rowptr, col = m.make_graph(50_000, 5_000, 500_000, 0)
    return rowptr.astype(np.int64), col.astype(np.int32)


def test_hit_share_into_users_is_twice_the_min_column_order():
    """One chunk per XCD part. Modelled here: min column 10.27 %, greedy placed 21.6 %."""
    m = _model()
    rowptr, col = _model_graph()
    U, I, window = 50_000, 5_000, 81
    ordered = m.hit_share(rowptr, col, m.min_column_order(rowptr, col, I), window)
    order = greedy(rowptr, col, I, window=window, cap=1024, R=m.ROWS_PER_WG, xcds=m.XCDS,
                   chunks=1, threads=0)
    assert _is_permutation(order, U)
    got = m.hit_share(rowptr, col, order, window)
    print(f"into users: min column {100 * ordered:.2f} %, greedy placed {100 * got:.2f} %")
    assert 0.09 < ordered < 0.12
    assert got >= 2 * ordered


def test_hit_share_of_a_block_into_items_is_twice_the_min_column_order():
    """Block 0 of 4 of the transposed graph. Modelled here: min column 3.18 %, greedy 6.78 %."""
    m = _model()
    rowptr, col = _model_graph()
    U, I, window, P = 50_000, 5_000, 81, 4
    cptr, crow = m.transpose(rowptr, col, I)
    cut = U // P
    keep = crow < cut
    bptr = np.concatenate([[0], np.cumsum(keep)])[cptr]
    bcol = crow[keep]
    ordered = m.hit_share(bptr, bcol, m.min_column_order(bptr, bcol, cut), window)
    order = greedy_blocks(cptr.astype(np.int64), crow.astype(np.int32), U, P, window=window,
                          cap=1024, R=m.ROWS_PER_WG, xcds=m.XCDS, chunks=1, threads=0)[0]
    assert _is_permutation(order, I)
    got = m.hit_share(bptr, bcol, order, window)
    print(f"into items, block 0 of {P}: min column {100 * ordered:.2f} %, greedy {100 * got:.2f} %")
    assert 0.025 < ordered < 0.04
    assert got >= 2 * ordered


def test_geometry_and_kind_rule():
    lib = nat.load()
    rows, window = ctypes.c_int32(0), ctypes.c_int64(0)

    def geom(d, blocked):
        assert lib.hgd_spmm_order_geometry(d, blocked, ctypes.byref(rows), ctypes.byref(window))
        return rows.value, window.value

    # a group of d / 4 lanes per row in a workgroup of 256; 4 MiB of the rows one pass gathers
    assert geom(64, 0) == (16, 16384) and geom(64, 1) == (16, 16384)
    assert geom(128, 0) == (8, 8192) and geom(128, 1) == (8, 8192)
    assert geom(32, 0) == (32, 32768)
    assert geom(256, 0) == (16, 16384)  # 64-column passes
    assert geom(256, 1) == (8, 8192)  # a blocked hop's 128-column passes
    assert not lib.hgd_spmm_order_geometry(0, 0, ctypes.byref(rows), ctypes.byref(window))
    U, I, E = 10_000_000, 1_000_000, 100_000_000
    kind = lib.hgd_spmm_row_order_kind_for
    assert kind(U, I, E, 64, 0) == nat.ORDER_GREEDY and kind(I, U, E, 64, 4) == nat.ORDER_GREEDY
    assert kind(I, U, E, 64, 0) == nat.ORDER_NONE  # 100 nonzeros a row
    assert kind(6_040, 3_706, 750_000, 64, 0) == nat.ORDER_NONE
    for n, m_, e, d, p in ((U, I, E, 32, 0), (U, I, E, 128, 1), (I, U, E, 128, 8),
                           (I, U, E, 64, 3), (I, U, E, 64, 100), (100, 1000, 500, 8, 3)):
        on = lib.hgd_spmm_block_order_for(n, m_, e, d, p) if p > 1 else \
            lib.hgd_spmm_row_order_for(n, m_, e, d)
        assert kind(n, m_, e, d, p) == (nat.ORDER_GREEDY if on else nat.ORDER_NONE)


def test_order_kind_environment(monkeypatch):
    import torch
    from hypergraph_diffusion_for_recommendation_amd.incidence import (CSR, order_geometry,
                                                                      spmm_order_kind)

    def csr(n_rows, n_cols, nnz):
        s = CSR(torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), n_rows,
                n_cols, split_threshold=0)
        s.nnz = nnz
        s.persistent = True  # (what Incidence.persist says of a structure that lasts)
        return s

    monkeypatch.delenv("HGD_SPMM_ORDER_KIND", raising=False)
    monkeypatch.delenv("HGD_SPMM_ORDER_PLACE", raising=False)
    big, small = csr(10_000_000, 1_000_000, 100_000_000), csr(100, 1000, 500)
    assert spmm_order_kind(big, 64) == nat.ORDER_GREEDY
    assert spmm_order_kind(csr(1_000_000, 10_000_000, 100_000_000), 64, 4) == nat.ORDER_GREEDY
    # a hop ordered only because the environment forces it: the min-column order
    assert spmm_order_kind(small, 8) == nat.ORDER_MIN_COLUMN
    monkeypatch.setenv("HGD_SPMM_ORDER_KIND", "2")
    assert spmm_order_kind(small, 8) == nat.ORDER_GREEDY
    monkeypatch.setenv("HGD_SPMM_ORDER_KIND", "1")
    assert spmm_order_kind(big, 64) == nat.ORDER_MIN_COLUMN
    monkeypatch.setenv("HGD_SPMM_ORDER_KIND", "auto")
    assert spmm_order_kind(big, 64) == nat.ORDER_GREEDY
    for bad in ("0", "3", "greedy", " 2"):
        monkeypatch.setenv("HGD_SPMM_ORDER_KIND", bad)
        with pytest.raises(ValueError):
            spmm_order_kind(big, 64)
    assert order_geometry(64, False) == (16384, 16, 8, 1)
    monkeypatch.setenv("HGD_SPMM_ORDER_PLACE", "0")
    assert order_geometry(64, True) == (16384, 16, 1, 8)
    monkeypatch.setenv("HGD_SPMM_ORDER_PLACE", "2")
    with pytest.raises(ValueError):
        order_geometry(64, False)


def test_only_a_persistent_structure_takes_the_greedy_order(monkeypatch):
    """The greedy build copies the structure to the host and synchronises the stream: a structure
    made per step (Incidence.drop's, possibly inside a captured step) must never pay it, whatever
    the size rule and the environment say. A CSR does not persist until Incidence.persist (or a
    ShardedIncidence over it) says so."""
    import torch
    from hypergraph_diffusion_for_recommendation_amd import incidence
    from hypergraph_diffusion_for_recommendation_amd.incidence import (CSR, Incidence,
                                                                      spmm_order_kind)
    monkeypatch.delenv("HGD_SPMM_ORDER_KIND", raising=False)
    U, I, E = 10_000_000, 1_000_000, 100_000_000

    def csr(n_rows, n_cols):
        s = CSR(torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), n_rows,
                n_cols, split_threshold=0)
        s.nnz = E
        return s

    inc = Incidence(csr(U, I), csr(I, U), None, None)
    assert not inc.csr.persistent and not inc.csc.persistent
    for env in (None, "auto", "2"):
        if env is not None:
            monkeypatch.setenv("HGD_SPMM_ORDER_KIND", env)
        assert spmm_order_kind(inc.csr, 64) == nat.ORDER_MIN_COLUMN
        assert spmm_order_kind(inc.csc, 64, 4) == nat.ORDER_MIN_COLUMN
    monkeypatch.setenv("HGD_SPMM_ORDER_KIND", "3")  # (still parsed strictly)
    with pytest.raises(ValueError):
        spmm_order_kind(inc.csr, 64)
    monkeypatch.delenv("HGD_SPMM_ORDER_KIND")
    assert inc.persist() is inc and inc.csr.persistent and inc.csc.persistent
    assert spmm_order_kind(inc.csr, 64) == nat.ORDER_GREEDY
    assert spmm_order_kind(inc.csc, 64, 4) == nat.ORDER_GREEDY
    # a sharded graph is the run's graph
    from hypergraph_diffusion_for_recommendation_amd.sharded import ShardedIncidence
    other = Incidence(csr(U, I), csr(I, U), None, None)
    monkeypatch.setattr(ShardedIncidence, "_global_col_scale", lambda self, Q: None)
    ShardedIncidence(other)
    assert other.csr.persistent and other.csc.persistent
    # a greedy order is one of a geometry: none is assumed
    with pytest.raises(ValueError, match="order_geometry"):
        inc.csr.row_order(nat.ORDER_GREEDY)
    with pytest.raises(ValueError, match="order_geometry"):
        inc.csc.col_blocks_ordered(4, nat.ORDER_GREEDY)
    assert incidence._need_geom((64, 16, 8, 1)) == (64, 16, 8, 1)


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_stand_alone_program_runs_clean_under_sanitizers(tmp_path, sanitizers):
    """csrc/row_order_greedy.cpp with tests/native/row_order_greedy_main.cpp (its own main; not
    loaded into Python), over the shapes above with 1, 2 and 7 threads."""
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
    exe = str(tmp_path / "row_order_greedy")
    src = [os.path.join(ROOT, "hypergraph_diffusion_for_recommendation_amd", "csrc",
                        "row_order_greedy.cpp"),
           os.path.join(ROOT, "tests", "native", "row_order_greedy_main.cpp")]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={sanitizers}",
                          "-fno-sanitize-recover=all", "-o", exe] + src, check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout
    assert "all orders are permutations" in run.stdout
    assert "Sanitizer" not in run.stdout and "runtime error" not in run.stdout
