"""Host logic of the block order's selection (incidence.spmm_block_order and the library's size
rule hgd_spmm_block_order_for), and which hops spmm_csr sends to hgd_spmm_blocked_ordered. No
GPU: the structures are CPU tensors that are never launched on."""
import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from hypergraph_diffusion_for_recommendation_amd import incidence
from hypergraph_diffusion_for_recommendation_amd.incidence import CSR, spmm_block_order

U, I, E = 10_000_000, 1_000_000, 100_000_000  # the bench shape; the hop into items gathers U rows
# what the measurement between the rule's two bounds said: the hop into items is
# 1.4 % faster at d = 64, P = 4 and 3.9 % at d = 128, P = 8, beyond the rounds' spread
MEASURED_ON = 1


def _csr(n_rows, n_cols, nnz):
    # (the arrays are never read: one element stands for nnz of them)
    rowptr = torch.zeros(2, dtype=torch.int64)
    s = CSR(rowptr, torch.zeros(1, dtype=torch.int32), n_rows, n_cols, split_threshold=0)
    s.nnz = nnz
    s.cols_ascending = True
    return s


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("HGD_SPMM_BLOCK_ORDER", raising=False)
    monkeypatch.delenv("HGD_SPMM_BLOCKS", raising=False)


def test_rule_at_the_bench_shape():
    """The measurement decides between the two bounds; what it said is pinned
    here: MEASURED_ON."""
    f, blocks_for = nat.load().hgd_spmm_block_order_for, nat.load().hgd_spmm_blocks_for
    assert blocks_for(U, 64) == 4 and blocks_for(U, 128) == 8
    assert f(I, U, E, 64, 4) == MEASURED_ON
    assert f(I, U, E, 128, 8) == MEASURED_ON
    assert spmm_block_order(_csr(I, U, E), 64, 4) == bool(MEASURED_ON)


def test_rule_bounds():
    f = nat.load().hgd_spmm_block_order_for
    for bad in ((0, U, E, 64, 4), (I, 0, E, 64, 4), (I, U, 0, 64, 4), (I, U, E, 0, 4),
                (I, U, E, 64, 0), (-1, U, E, 64, 4), (I, U, E, 64, -2)):
        assert f(*bad) == 0
    # the 32 MiB step of the slice one pass gathers from: n_src_rows / P rows of 4·min(d, 128) B
    n = (32 << 20) // 256
    assert f(I, 4 * n - 4, E, 64, 4) == 0
    assert f(I, 8 * (n // 2) - 8, E, 128, 8) == 0 and f(I, 8 * (n // 2) - 8, E, 256, 8) == 0
    assert f(I, U, E, 64, 100) == 0  # 100 K-row slices of 25.6 MB
    # above 32 nonzeros per piece the order is off whatever the slice
    assert f(I, U, 32 * 4 * I + 1, 64, 4) == 0
    assert f(I, U, E, 64, 3) == 0  # 33.3 a piece
    assert f(I, U, 33 * 8 * I, 128, 8) == 0


def test_environment_override(monkeypatch):
    small = _csr(100, 1000, 500)
    assert not spmm_block_order(small, 8, 3)
    assert spmm_block_order(_csr(I, U, E), 64, 4)
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "1")
    assert spmm_block_order(small, 8, 3)
    assert not spmm_block_order(small, 8, 0) and not spmm_block_order(small, 8, 1)  # not blocked
    assert not spmm_block_order(_csr(100, 1000, 0), 8, 3)
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "0")
    assert not spmm_block_order(_csr(I, U, E), 64, 4)
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "auto")
    assert not spmm_block_order(small, 8, 3)
    for bad in ("2", "on", "-1", " 1"):
        monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", bad)
        with pytest.raises(ValueError):
            spmm_block_order(small, 8, 3)


class _Stop(Exception):
    pass


class _Lib:
    """Stands for libhgd: records the hop entry point spmm_csr calls, then stops the call."""

    def __init__(self, real):
        self._real = real
        self.called = []

    def __getattr__(self, name):
        if name.startswith("hgd_spmm") and "workspace" not in name and not name.endswith(
                ("_for", "_for_dt")):
            def hop(*a):
                self.called.append(name)
                raise _Stop
            return hop
        return getattr(self._real, name)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the device: spmm_csr's argument checks pass and the
    recorded entry point is reached without one."""

    @property
    def device(self):
        return torch.device("cuda:0")


def _hop_taken(monkeypatch, csr, X, **kw):
    lib = _Lib(nat.load())
    monkeypatch.setattr(incidence.nat, "load", lambda: lib)
    monkeypatch.setattr(incidence, "_stream", lambda dev: None)
    monkeypatch.setattr(incidence, "_ws", lambda n, dev: torch.empty(max(int(n), 1),
                                                                     dtype=torch.uint8))
    empty32 = torch.zeros(1, dtype=torch.int32)
    empty64 = torch.zeros(1, dtype=torch.int64)
    csr._col_blocks_ord[3] = (empty64, empty32, empty32, empty32)
    csr._col_blocks[3] = (empty64, empty32, empty32)
    with pytest.raises(_Stop):
        incidence.spmm_csr(csr, X, **kw)
    return lib.called[-1]


def test_only_the_plain_fp32_blocked_hop_over_all_rows_takes_the_order(monkeypatch):
    """With the order and three blocks forced: the fp32 hop over all rows is
    hgd_spmm_blocked_ordered; a bf16 table, a row range, a mask and a fused epilogue are the
    entry points they were."""
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "1")
    R, C, d = 40, 30, 8
    out = torch.zeros(R, d).as_subclass(_FakeCuda)

    def X(dtype=torch.float32):
        return torch.zeros(C, d, dtype=dtype).as_subclass(_FakeCuda)

    csr = _csr(R, C, 200)
    assert _hop_taken(monkeypatch, csr, X(), out=out) == "hgd_spmm_blocked_ordered"
    assert _hop_taken(monkeypatch, csr, X(), out=out, row_begin=1) == "hgd_spmm_blocked"
    assert _hop_taken(monkeypatch, csr, X(), out=out, row_end=R - 1) == "hgd_spmm_blocked"
    out16 = torch.zeros(R, d, dtype=torch.bfloat16).as_subclass(_FakeCuda)
    assert _hop_taken(monkeypatch, csr, X(torch.bfloat16), out=out16) == "hgd_spmm_blocked_dt"
    assert _hop_taken(monkeypatch, csr, X(), out=out16) == "hgd_spmm_blocked_dt"
    assert _hop_taken(monkeypatch, csr, X(torch.bfloat16), out=out) == "hgd_spmm_blocked_dt"
    assert _hop_taken(monkeypatch, csr, X(), out=out, ex=nat.RowEpilogue()) == "hgd_spmm_fused"
    assert _hop_taken(monkeypatch, csr, X(), out=out, blocks=0) == "hgd_spmm"
    masked = _csr(R, C, 200)
    masked.mask, masked.keep = torch.ones(200, dtype=torch.uint8), 0.5
    assert _hop_taken(monkeypatch, masked, X(), out=out) == "hgd_spmm_masked"
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "0")
    assert _hop_taken(monkeypatch, csr, X(), out=out) == "hgd_spmm_blocked"


def test_block_ordered_implementation_bytes():
    from hypergraph_diffusion_for_recommendation_amd import profiling
    nnz, R, d, P = 1000, 100, 64, 4
    blocked = profiling.impl_bytes(nnz, R, d, True, True, P)
    assert profiling.impl_bytes(nnz, R, d, True, True, P, block_ordered=True) == blocked + 4 * R * P
    assert profiling.impl_bytes(nnz, R, d, True, True, P, block_ordered=False) == blocked
    # the keyword counts nothing on a hop that is not blocked, and hop_bytes has no such term
    plain = profiling.impl_bytes(nnz, R, d, True, True)
    assert profiling.impl_bytes(nnz, R, d, True, True, block_ordered=True) == plain
    assert profiling.hop_bytes(nnz, R, d) == nnz * (4 + 4 * d) + R * (4 * d + 4) + (R + 1) * 4

