"""Host logic of the ordered hop's selection (incidence.spmm_row_order and the library's size
rule hgd_spmm_row_order_for). No GPU: the structures are CPU tensors that are never launched
on."""
import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from hypergraph_diffusion_for_recommendation_amd.incidence import CSR, spmm_row_order


def _csr(n_rows, n_cols, nnz):
    # (the arrays are never read: one element stands for nnz of them)
    rowptr = torch.zeros(2, dtype=torch.int64)
    s = CSR(rowptr, torch.zeros(1, dtype=torch.int32), n_rows, n_cols, split_threshold=0)
    s.nnz = nnz
    return s


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("HGD_SPMM_ROW_ORDER", raising=False)


def test_rule_at_the_bench_shape():
    f = nat.load().hgd_spmm_row_order_for
    U, I, E = 10_000_000, 1_000_000, 100_000_000
    # into users: 10 nonzeros a row from the 256 MB item table — measured −8 % ordered at
    # d = 32, 64 and 128
    assert f(U, I, E, 64) == 1 and f(U, I, E, 32) == 1 and f(U, I, E, 128) == 1
    assert spmm_row_order(_csr(U, I, E), 64)
    # into items: 100 nonzeros a row, one gather in 100 to turn
    assert f(I, U, E, 64) == 0
    assert not spmm_row_order(_csr(I, U, E), 64)


@pytest.mark.parametrize("users,items,edges", [(6_040, 3_706, 750_000),
                                               (31_668, 38_048, 1_170_000),
                                               (52_643, 91_599, 2_240_000)])
def test_rule_is_off_when_the_table_fits_the_aggregate_l2(users, items, edges):
    f = nat.load().hgd_spmm_row_order_for
    for d in (32, 64):
        assert f(users, items, edges, d) == 0 and f(items, users, edges, d) == 0
    assert not spmm_row_order(_csr(users, items, edges), 64)


def test_rule_bounds():
    f = nat.load().hgd_spmm_row_order_for
    assert f(0, 1_000_000, 10, 64) == 0 and f(10, 0, 10, 64) == 0
    assert f(10, 1_000_000, 0, 64) == 0 and f(10, 1_000_000, 10, 0) == 0
    # the 32 MiB step of the table one pass gathers from (d·4 bytes a row up to d = 128, 64-column
    # passes beyond)
    n = (32 << 20) // 256
    assert f(10 * n, n - 1, 100 * n, 64) == 0
    assert f(10 * n, n - 1, 100 * n, 256) == 0
    # above an average row length of 32 the order is off whatever the table
    U, I = 10_000_000, 1_000_000
    assert f(U, I, 32 * U + 1, 64) == 0
    assert f(U, I, 33 * U, 128) == 0


def test_only_for_unsplit_row_walks(monkeypatch):
    U, I, E = 10_000_000, 1_000_000, 100_000_000
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "1")  # forcing never overrides the structure rules
    assert spmm_row_order(_csr(U, I, E), 64)
    assert not spmm_row_order(_csr(U, I, 0), 64)
    s = _csr(U, I, E)
    s.plan.flags = 1  # the segmented walk
    assert not spmm_row_order(s, 64)
    s = _csr(U, I, E)
    s.plan.threshold, s.plan.n_heavy = 16, 3  # split rows
    assert not spmm_row_order(s, 64)


def test_environment_override(monkeypatch):
    small = _csr(100, 1000, 500)
    assert not spmm_row_order(small, 8)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "1")
    assert spmm_row_order(small, 8)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "0")
    assert not spmm_row_order(_csr(10_000_000, 1_000_000, 100_000_000), 64)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "auto")
    assert not spmm_row_order(small, 8)
    for bad in ("2", "on", "-1", " 1"):
        monkeypatch.setenv("HGD_SPMM_ROW_ORDER", bad)
        with pytest.raises(ValueError):
            spmm_row_order(small, 8)


def test_ordered_implementation_bytes():
    from hypergraph_diffusion_for_recommendation_amd import profiling
    nnz, R, d = 1000, 100, 64
    plain = profiling.impl_bytes(nnz, R, d, True, True)
    assert profiling.impl_bytes(nnz, R, d, True, True, ordered=True) == plain + 4 * R
