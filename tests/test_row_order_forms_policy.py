"""Host logic of the row order of the fused, masked and 16-bit hops: the geometry and rule
queries of a form (hgd_spmm_order_geometry_dt, hgd_spmm_row_order_for_dt) against the launcher's
pass plan written out by hand, incidence.spmm_row_order / order_geometry with their keyword
arguments, the environment overrides and the implementation bytes. No GPU: the structures are
CPU tensors that are never launched on."""
import ctypes

import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from hypergraph_diffusion_for_recommendation_amd import profiling
from hypergraph_diffusion_for_recommendation_amd.incidence import (CSR, order_geometry,
                                                                    spmm_row_order)

F32, BF16 = nat.DT_F32, nat.DT_BF16
T32, T16 = torch.float32, torch.bfloat16
L2 = 4 << 20  # an XCD's L2: the window counts the gathered pieces it holds
BLOCK = 256   # threads of a workgroup: rows per workgroup = BLOCK / lanes per row

# (x, y, fused) -> {d: (lanes per row, columns per pass)}: a lane owns 4 columns of an all-fp32
# hop (16 bytes) and 8 with a 16-bit side; an fp32 row up to 128 columns is one pass and a wider
# one runs in 64-column passes, a row with a 16-bit side in 128-column passes, and a fused row is
# one pass (up to 256 columns: 64 lanes in fp32, 32 with 8-column lanes)
PLAN = {
    (F32, F32, 0): {64: (16, 64), 128: (32, 128), 256: (16, 64)},
    (F32, F32, 1): {64: (16, 64), 128: (32, 128), 256: (64, 256)},
    (BF16, BF16, 0): {64: (8, 64), 128: (16, 128), 256: (16, 128)},
    (BF16, F32, 0): {64: (8, 64), 128: (16, 128), 256: (16, 128)},
    (F32, BF16, 0): {64: (8, 64), 128: (16, 128), 256: (16, 128)},
    (BF16, F32, 1): {64: (8, 64), 128: (16, 128), 256: (32, 256)},
}


def _geometry(d, blocked, x, y, fused):
    rows, window = ctypes.c_int32(-1), ctypes.c_int64(-1)
    ok = nat.load().hgd_spmm_order_geometry_dt(d, blocked, x, y, fused, ctypes.byref(rows),
                                               ctypes.byref(window))
    return ok, int(rows.value), int(window.value)


@pytest.mark.parametrize("form", list(PLAN), ids=lambda f: f"x{f[0]}y{f[1]}f{f[2]}")
@pytest.mark.parametrize("d", [64, 128, 256])
def test_geometry_is_the_pass_plan_of_the_form(form, d):
    x, y, fused = form
    lanes, pass_cols = PLAN[form][d]
    piece = pass_cols * (2 if x == BF16 else 4)  # bytes of a source row one pass gathers
    assert _geometry(d, 0, x, y, fused) == (1, BLOCK // lanes, L2 // piece)
    dt = {F32: T32, BF16: T16}
    assert order_geometry(d, False, dt[x], dt[y], bool(fused))[:2] == (L2 // piece, BLOCK // lanes)


def test_plain_form_answers_as_the_existing_query():
    lib = nat.load()
    for d in (4, 7, 32, 64, 96, 128, 256, 320):
        for blocked in (0, 1):
            rows, window = ctypes.c_int32(0), ctypes.c_int64(0)
            assert lib.hgd_spmm_order_geometry(d, blocked, ctypes.byref(rows), ctypes.byref(window))
            assert _geometry(d, blocked, F32, F32, 0) == (1, rows.value, window.value)
        assert order_geometry(d, False) == order_geometry(d, False, T32, T32, False)
    # the existing query's answers, unchanged
    rows, window = ctypes.c_int32(0), ctypes.c_int64(0)
    assert lib.hgd_spmm_order_geometry(64, 0, ctypes.byref(rows), ctypes.byref(window))
    assert (rows.value, window.value) == (16, 16384)
    assert lib.hgd_spmm_order_geometry(256, 1, ctypes.byref(rows), ctypes.byref(window))
    assert (rows.value, window.value) == (8, 8192)  # (a blocked hop: 128-column passes)


def test_geometry_bad_arguments():
    assert _geometry(0, 0, F32, F32, 0)[0] == 0
    assert _geometry(64, 0, 2, F32, 0)[0] == 0 and _geometry(64, 0, F32, -1, 0)[0] == 0
    assert _geometry(64, 0, BF16, BF16, 1)[0] == 0  # no fused hop into a 16-bit Y
    assert _geometry(64, 1, F32, F32, 1)[0] == 0    # nor over source blocks
    assert nat.load().hgd_spmm_order_geometry_dt(64, 0, F32, F32, 0, None, None) == 0
    # the unaligned path of the one-column lanes: d = 12 with 8-column lanes
    assert _geometry(12, 0, BF16, BF16, 0) == (1, 16, L2 // (12 * 2))


def _csr(n_rows, n_cols, nnz):
    rowptr = torch.zeros(2, dtype=torch.int64)
    s = CSR(rowptr, torch.zeros(1, dtype=torch.int32), n_rows, n_cols, split_threshold=0)
    s.nnz = nnz
    return s


FORMS = [dict(fused=True), dict(masked=True), dict(masked=True, fused=True),
         dict(x_dtype=T16, y_dtype=T16), dict(x_dtype=T16), dict(y_dtype=T16),
         dict(x_dtype=T16, masked=True), dict(x_dtype=T16, fused=True),
         dict(x_dtype=T16, fused=True, masked=True)]
BENCH = (10_000_000, 1_000_000, 100_000_000)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("HGD_SPMM_ROW_ORDER", raising=False)


def test_rule_of_the_plain_form_is_the_existing_rule():
    lib = nat.load()
    for n, m, e in (BENCH, BENCH[1::-1] + BENCH[2:], (6_040, 3_706, 750_000),
                    (52_643, 91_599, 2_240_000)):
        for d in (32, 64, 128, 256):
            assert (lib.hgd_spmm_row_order_for_dt(n, m, e, d, F32, F32, 0, 0)
                    == lib.hgd_spmm_row_order_for(n, m, e, d))
    assert lib.hgd_spmm_row_order_for(*BENCH, 64) == 1  # (unchanged)
    assert spmm_row_order(_csr(*BENCH), 64) and not spmm_row_order(_csr(100, 1000, 500), 8)
    assert lib.hgd_spmm_row_order_for_dt(*BENCH, 64, 2, F32, 0, 0) == 0  # unknown dtype code


def test_rules_that_the_measurement_turned_on():
    """at the bench graph's hop into users the ordered twin beat the unordered
    call, in the min-column and in the greedy order, for the fp32 fused hop and for the plain
    bf16 hop at d = 128 — and for nothing else that was measured."""
    f = nat.load().hgd_spmm_row_order_for_dt
    U, I, E = BENCH
    assert f(U, I, E, 128, F32, F32, 1, 0) == 1   # fused fp32
    assert f(U, I, E, 128, BF16, BF16, 0, 0) == 1  # the plain bf16 hop
    assert spmm_row_order(_csr(U, I, E), 128, fused=True)
    assert spmm_row_order(_csr(U, I, E), 128, x_dtype=T16, y_dtype=T16)
    # the Amazon-Book encoder shape of BASELINE configs[3] (144,242 rows each way)
    n = 52_643 + 91_599
    assert f(n, n, 2 * 2_240_000, 128, F32, F32, 1, 0) == 1
    # the same forms at the width they lost or stayed inside the ranges at, and unmeasured ones
    for d in (32, 64, 96, 256):
        assert f(U, I, E, d, F32, F32, 1, 0) == 0 and f(U, I, E, d, BF16, BF16, 0, 0) == 0
    # the forms that lost: fused bf16, everything masked; the unmeasured dtype pairs
    for x, y, fused, masked in ((BF16, F32, 1, 0), (F32, F32, 0, 1), (F32, F32, 1, 1),
                                (BF16, BF16, 0, 1), (BF16, F32, 1, 1), (BF16, F32, 0, 0),
                                (F32, BF16, 0, 0)):
        assert f(U, I, E, 128, x, y, fused, masked) == 0, (x, y, fused, masked)
    # inside the plain rule's bounds only: the table in the form's element size under 32 MiB
    # (bf16 rows of 128 are 256 B: 131,072 of them), long rows, and the control's Yelp shape
    assert f(10 * 131_071, 131_071, 100 * 131_071, 128, BF16, BF16, 0, 0) == 0
    assert f(10 * 131_072, 131_072, 100 * 131_072, 128, BF16, BF16, 0, 0) == 1
    assert f(10 * 65_535, 65_535, 100 * 65_535, 128, F32, F32, 1, 0) == 0
    assert f(10 * 65_536, 65_536, 100 * 65_536, 128, F32, F32, 1, 0) == 1
    assert f(U, I, 32 * U + 1, 128, F32, F32, 1, 0) == 0
    assert f(69_716, 69_716, 2_470_000, 64, F32, F32, 1, 0) == 0
    assert f(0, I, E, 128, F32, F32, 1, 0) == 0 and f(U, I, 0, 128, BF16, BF16, 0, 0) == 0


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "-".join(sorted(f)))
def test_rule_of_a_form_never_orders_where_the_plain_rule_does_not(form):
    """A form's rule is set by measurement inside the region the plain rule orders: wherever the
    plain fp32 hop stays unordered (the table fits the aggregate L2, or the rows are long) every
    form stays unordered too."""
    for n, m, e in ((6_040, 3_706, 750_000), (31_668, 38_048, 1_170_000),
                    (1_000_000, 10_000_000, 100_000_000)):
        for d in (64, 128):
            assert not spmm_row_order(_csr(n, m, e), d)
            assert not spmm_row_order(_csr(n, m, e), d, **form)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "-".join(sorted(f)))
def test_environment_governs_every_form(monkeypatch, form):
    small, big = _csr(100, 1000, 500), _csr(*BENCH)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "1")
    assert spmm_row_order(small, 64, **form) and spmm_row_order(big, 64, **form)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "0")
    assert not spmm_row_order(small, 64, **form) and not spmm_row_order(big, 64, **form)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "auto")
    assert not spmm_row_order(small, 64, **form)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "on")
    with pytest.raises(ValueError):
        spmm_row_order(small, 64, **form)
    # forcing never overrides the structure rules
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "1")
    assert not spmm_row_order(_csr(100, 1000, 0), 64, **form)
    s = _csr(*BENCH)
    s.plan.flags = 1  # the segmented walk
    assert not spmm_row_order(s, 64, **form)
    s = _csr(*BENCH)
    s.plan.threshold, s.plan.n_heavy = 16, 3  # split rows
    assert not spmm_row_order(s, 64, **form)
    s = _csr(*BENCH)
    s.row_order_ok = False  # a structure that opted out (a KG attention pattern)
    assert not spmm_row_order(s, 64, **form) and not spmm_row_order(s, 64)


def test_masked_view_takes_its_orders_from_the_parent():
    import copy
    parent = _csr(100, 1000, 500)
    assert parent.order_source() is parent
    view = copy.copy(parent)
    view._order_parent = parent
    assert view.order_source() is parent
    again = copy.copy(view)  # a view of a view: still the structure itself
    assert again.order_source() is parent


def test_ordered_forms_implementation_bytes():
    nnz, R, d = 1000, 100, 64
    for xb, yb in ((4, 4), (2, 2), (2, 4), (4, 2)):
        plain = profiling.impl_bytes(nnz, R, d, True, True, x_bytes=xb, y_bytes=yb)
        assert plain == nnz * (8 + xb * d) + R * (yb * d + 4) + (R + 1) * 8
        got = profiling.impl_bytes(nnz, R, d, True, True, x_bytes=xb, y_bytes=yb, ordered=True)
        assert got == plain + 4 * R  # the row id of every row
    assert (profiling.impl_bytes(nnz, R, d, False, False, x_bytes=2, ordered=True)
            == nnz * (4 + 2 * d) + R * 4 * d + (R + 1) * 8 + 4 * R)
