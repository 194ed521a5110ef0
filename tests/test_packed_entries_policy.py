"""Host logic of the packed entries of the block-ordered hop (one word per nonzero: block-local
column + weight code): the library's rule hgd_spmm_packed_for and fit test hgd_spmm_packed_fits at
the bench shape and at the bit limits, incidence.spmm_packed's reading of HGD_SPMM_PACKED, what
hgd_spmm_blocked_packed and hgd_spmm_pack_entries answer to a call they reject, which entry point
spmm_csr takes with and without ``src_scale``, and profiling.impl_bytes' keyword. No GPU: the
structures are CPU tensors that are never launched on and the rejected calls return before the
first HIP call."""
import weakref

import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from hypergraph_diffusion_for_recommendation_amd import incidence
from hypergraph_diffusion_for_recommendation_amd.incidence import CSR, spmm_packed

U, I, E = 10_000_000, 1_000_000, 100_000_000  # the bench shape; the hop into items gathers U rows
BITS = nat.PACKED_IDX_BITS
OK, INVALID, UNSUPPORTED = 0, 1, 3


def _csr(n_rows, n_cols, nnz):
    # (the arrays are never read: one element stands for nnz of them)
    rowptr = torch.zeros(2, dtype=torch.int64)
    s = CSR(rowptr, torch.zeros(1, dtype=torch.int32), n_rows, n_cols, split_threshold=0)
    s.nnz = nnz
    s.cols_ascending = True
    return s


def _prime(csr, blocks, scale, n_dict):
    """Stands for CSR.packed_entries' device build: its cache entry for ``scale``."""
    got = (torch.zeros(1, dtype=torch.int32), torch.zeros(max(n_dict, 1)), n_dict)
    csr._packed[(blocks, BITS, id(scale))] = (weakref.ref(scale), scale._version, got)
    return got


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for name in ("HGD_SPMM_PACKED", "HGD_SPMM_BLOCK_ORDER", "HGD_SPMM_BLOCKS"):
        monkeypatch.delenv(name, raising=False)


def test_constants_are_the_headers():
    text = open(__file__.rsplit("/tests/", 1)[0] + "/include/hgd.h").read()
    assert f"#define HGD_SPMM_PACKED_IDX_BITS {nat.PACKED_IDX_BITS}\n" in text
    assert f"#define HGD_SPMM_PACKED_MAX_DICT {nat.PACKED_MAX_DICT}\n" in text


def test_rule_at_the_bench_shape():
    """Poisson(10) user degrees are a few dozen distinct scales; the blocks are the size rule's."""
    lib = nat.load()
    f = lib.hgd_spmm_packed_for
    assert lib.hgd_spmm_blocks_for(U, 64) == 4 and lib.hgd_spmm_blocks_for(U, 128) == 8
    for n_dict in (1, 40, 1024):
        assert f(U, 4, n_dict, BITS) == 1 and f(U, 8, n_dict, BITS) == 1
    assert f(U, 4, 1025, BITS) == 0
    # the hop into users gathers the 1 M item rows: never blocked, and one block is no blocked hop
    assert lib.hgd_spmm_blocks_for(I, 64) == 0 and f(I, 0, 40, BITS) == 0 and f(I, 1, 40, BITS) == 0


def test_rule_at_the_bit_limits():
    lib = nat.load()
    f, fits = lib.hgd_spmm_packed_for, lib.hgd_spmm_packed_fits
    # a block of exactly 2^idx_bits source rows, and one more (the widest block is the ceiling)
    for bits, P in ((22, 4), (22, 3), (16, 2), (20, 64)):
        n = P << bits
        assert f(n, P, 1, bits) == 1 and fits(n, P, 1, bits) == 1
        assert f(n + 1, P, 1, bits) == 0 and fits(n + 1, P, 1, bits) == 0
        assert fits(n - P + 1, P, 1, bits) == 1  # (⌈n / P⌉ is still 2^bits)
    # dictionaries of 1, 2^(32 − idx_bits) and one more entries
    for bits in (22, 24, 31):
        full = 1 << (32 - bits)
        n = 2 << 16
        assert f(n, 2, 1, bits) == 1 and f(n, 2, full, bits) == 1 and f(n, 2, full + 1, bits) == 0
        assert f(n, 2, 0, bits) == 0
    # ... but never more than the LDS copy holds, however many bits are left for the code
    assert f(2 << 16, 2, 1024, 16) == 1 and f(2 << 16, 2, 1025, 16) == 0
    assert fits(32, 2, 1024, 4) == 1 and fits(32, 2, 1025, 4) == 0
    # the fit at small sizes (the GPU tests' idx_bits = 4: blocks of exactly 16 rows, then 17),
    # where the rule is off: blocks under 65,536 source rows were forced, not chosen by size
    assert fits(32, 2, 2, 4) == 1 and fits(33, 2, 2, 4) == 0 and fits(34, 2, 2, 4) == 0
    assert fits(48, 3, 2, 4) == 1 and fits(49, 3, 2, 4) == 0
    assert f(32, 2, 2, 4) == 0 and f(2 * 65536 - 1, 2, 2, BITS) == 0 and f(2 * 65536, 2, 2, BITS) == 1
    # out of range arguments
    for bad in ((0, 4, 1, BITS), (-1, 4, 1, BITS), (U, 65, 1, BITS), (U, -1, 1, BITS),
                (U, 4, 1, 0), (U, 4, 1, 32), (U, 4, 1, -3), (U, 4, -1, BITS)):
        assert f(*bad) == 0
        assert fits(*bad) == 0 or bad[0] == 0  # (no source rows fit any format)


def test_environment_override(monkeypatch):
    small, big = _csr(100, 1000, 500), _csr(I, U, E)
    s_small, s_big = torch.ones(1000), torch.ones(U // 1000)  # (never read: the cache is primed)
    got_small, got_big = _prime(small, 3, s_small, 2), _prime(big, 4, s_big, 40)
    assert spmm_packed(small, 3, s_small) is None  # forced blocks of 333 rows: the rule is off
    assert spmm_packed(big, 4, s_big) is got_big
    assert spmm_packed(big, 4, None) is None  # no statement about the weights: nothing to pack
    monkeypatch.setenv("HGD_SPMM_PACKED", "1")
    assert spmm_packed(small, 3, s_small) is got_small
    assert spmm_packed(small, 0, s_small) is None and spmm_packed(small, 1, s_small) is None
    assert spmm_packed(_csr(100, 1000, 0), 3, s_small) is None
    assert spmm_packed(small, 3, None) is None
    monkeypatch.setenv("HGD_SPMM_PACKED", "0")
    assert spmm_packed(big, 4, s_big) is None
    monkeypatch.setenv("HGD_SPMM_PACKED", "auto")
    assert spmm_packed(small, 3, s_small) is None and spmm_packed(big, 4, s_big) is got_big
    for bad in ("2", "on", "-1", " 1", "01"):
        monkeypatch.setenv("HGD_SPMM_PACKED", bad)
        with pytest.raises(ValueError, match="HGD_SPMM_PACKED must be 0 or 1"):
            spmm_packed(small, 3, s_small)


def test_a_dictionary_that_does_not_fit_is_the_weighted_hop(monkeypatch):
    big = _csr(I, U, E)
    s = torch.ones(3)
    big._packed[(4, BITS, id(s))] = (weakref.ref(s), s._version, None)  # what packed_entries keeps
    assert spmm_packed(big, 4, s) is None
    monkeypatch.setenv("HGD_SPMM_PACKED", "1")
    assert spmm_packed(big, 4, s) is None


# -- what the two entry points answer to a call they reject -------------------------------------
P = 16  # a fake, 16-byte aligned, never dereferenced pointer
FN = "hgd_spmm_blocked_packed"
ORDER = ["blk_start", "ent", "dict", "n_dict", "idx_bits", "blk_row_scale", "blk_out_row",
         "n_rows", "n_src_rows", "X", "ldx", "Y", "ldy", "d", "epilogue", "slope", "n_blocks",
         "stream"]
# a call the entry point would launch; each case below breaks it somewhere
VALID = dict(blk_start=P, ent=P, dict=P, n_dict=2, idx_bits=4, blk_row_scale=None, blk_out_row=P,
             n_rows=3, n_src_rows=32, X=P, ldx=64, Y=P, ldy=64, d=64, epilogue=0, slope=0.0,
             n_blocks=2, stream=None)
NULLS = dict(blk_start=None, ent=None, dict=None, blk_out_row=None, X=None, Y=None)


def _fit(blocks, rows, weights, bits):
    return (f"{blocks} blocks of {rows} source rows and {weights} weights do not fit {bits} + "
            f"{32 - bits} bits (at most 1024 weights)")


CASES = [
    (dict(blk_out_row=None), INVALID, "null blk_out_row"),
    (dict(blk_start=None), INVALID, "null blk_start"),
    (dict(n_blocks=0), INVALID, "blocks must be 1..64"),
    (dict(n_blocks=65), INVALID, "blocks must be 1..64"),
    (dict(idx_bits=0), INVALID, "idx_bits must be 1..31 (got 0)"),
    (dict(idx_bits=32), INVALID, "idx_bits must be 1..31 (got 32)"),
    (dict(n_dict=0), INVALID, "n_dict must be >= 1 (got 0)"),
    (dict(n_dict=-4), INVALID, "n_dict must be >= 1 (got -4)"),
    (dict(dict=None), INVALID, "null dict"),
    # a block of 17 source rows in 4 bits; the dictionary against the code bits and the LDS copy
    (dict(n_src_rows=33), UNSUPPORTED, _fit(2, 33, 2, 4)),
    (dict(n_src_rows=49, n_blocks=3), UNSUPPORTED, _fit(3, 49, 2, 4)),
    (dict(n_dict=1025), UNSUPPORTED, _fit(2, 32, 1025, 4)),
    (dict(n_dict=3, idx_bits=31), UNSUPPORTED, _fit(2, 32, 3, 31)),
    (dict(n_dict=1025, idx_bits=22), UNSUPPORTED, _fit(2, 32, 1025, 22)),
    # what every hop checks, after the entry point's own
    (dict(ldx=63), INVALID, "ldx/ldy must be >= d"),
    (dict(epilogue=3), INVALID, "bad epilogue 3"),
    (dict(d=0), INVALID, "d must be > 0 (got 0)"),
    (dict(n_src_rows=-1), INVALID, "negative sizes"),
    (dict(Y=None), INVALID, "null rowptr/Y"),
    (dict(X=None), INVALID, "null X"),
    # two faults: order / blocks / starts / bits / dictionary / fit, then the shared checks
    (dict(blk_out_row=None, idx_bits=0), INVALID, "null blk_out_row"),
    (dict(n_blocks=65, idx_bits=0, dict=None), INVALID, "blocks must be 1..64"),
    (dict(idx_bits=0, n_dict=0, dict=None), INVALID, "idx_bits must be 1..31 (got 0)"),
    (dict(n_dict=0, dict=None, n_src_rows=33), INVALID, "n_dict must be >= 1 (got 0)"),
    (dict(dict=None, n_src_rows=33), INVALID, "null dict"),
    (dict(n_src_rows=33, d=0), UNSUPPORTED, _fit(2, 33, 2, 4)),
    # no rows: nothing to launch, whatever the pointers (the format is still checked)
    (dict(NULLS, n_rows=0), OK, ""),
    (dict(NULLS, n_rows=0, n_src_rows=33), UNSUPPORTED, _fit(2, 33, 2, 4)),
    (dict(NULLS, n_rows=0, idx_bits=0), INVALID, "idx_bits must be 1..31 (got 0)"),
]


def _id(c):
    return ",".join(f"{k}={x}" for k, x in c[0].items())


def _call(fn, order, valid, over):
    v = dict(valid, **over)
    lib = nat.load()
    got = getattr(lib, fn)(*[v[k] for k in order])
    return got, lib.hgd_get_last_error_string().decode()


@pytest.mark.parametrize("over,status,text", CASES, ids=[_id(c) for c in CASES])
def test_hop_rejection(over, status, text):
    got, msg = _call(FN, ORDER, VALID, over)
    print(f"{FN}: status {got}, {msg!r}")
    assert (got, msg) == (status, f"{FN}: {text}" if text else "")


def test_no_case_reaches_a_launch():
    for over, status, _ in CASES:
        assert status != OK or dict(VALID, **over)["n_rows"] == 0, over
    for over, status, _ in B_CASES:
        assert status != OK or dict(B_VALID, **over)["nnz"] == 0, over


def test_accepted_call_clears_the_error_text():
    lib = nat.load()
    assert _call(FN, ORDER, VALID, dict(d=0))[0] == INVALID
    assert lib.hgd_get_last_error_string() != b""
    assert _call(FN, ORDER, VALID, dict(NULLS, n_rows=0)) == (OK, "")


BUILD = "hgd_spmm_pack_entries"
B_ORDER = ["blk_start", "blk_col", "src_code", "n_rows", "n_src_rows", "nnz", "n_blocks", "n_dict",
           "idx_bits", "ent", "stream"]
B_VALID = dict(blk_start=P, blk_col=P, src_code=P, n_rows=3, n_src_rows=32, nnz=5, n_blocks=2,
               n_dict=2, idx_bits=4, ent=P, stream=None)
B_NULLS = dict(blk_start=None, blk_col=None, src_code=None, ent=None)
B_CASES = [
    (dict(n_rows=-1), INVALID, "negative sizes"),
    (dict(n_src_rows=-1), INVALID, "negative sizes"),
    (dict(nnz=-1), INVALID, "negative sizes"),
    (dict(n_blocks=0), INVALID, "blocks must be 1..64"),
    (dict(n_blocks=65), INVALID, "blocks must be 1..64"),
    (dict(n_src_rows=2**31, idx_bits=31), INVALID, "n_src_rows >= 2^31"),
    (dict(idx_bits=0), INVALID, "idx_bits must be 1..31 (got 0)"),
    (dict(idx_bits=32), INVALID, "idx_bits must be 1..31 (got 32)"),
    (dict(n_dict=0), INVALID, "n_dict must be >= 1 (got 0)"),
    (dict(n_src_rows=33), UNSUPPORTED, _fit(2, 33, 2, 4)),
    (dict(n_dict=1025), UNSUPPORTED, _fit(2, 32, 1025, 4)),
    (dict(n_dict=5, idx_bits=30, n_blocks=1), UNSUPPORTED, _fit(1, 32, 5, 30)),
    (dict(blk_start=None), INVALID, "null blk_start / blk_col / src_code / ent"),
    (dict(blk_col=None), INVALID, "null blk_start / blk_col / src_code / ent"),
    (dict(src_code=None), INVALID, "null blk_start / blk_col / src_code / ent"),
    (dict(ent=None), INVALID, "null blk_start / blk_col / src_code / ent"),
    (dict(n_blocks=0, idx_bits=0, n_src_rows=33), INVALID, "blocks must be 1..64"),
    (dict(idx_bits=0, n_dict=0), INVALID, "idx_bits must be 1..31 (got 0)"),
    (dict(n_src_rows=33, ent=None), UNSUPPORTED, _fit(2, 33, 2, 4)),
    (dict(B_NULLS, nnz=0), OK, ""),
    (dict(B_NULLS, nnz=0, n_src_rows=33), UNSUPPORTED, _fit(2, 33, 2, 4)),
]


@pytest.mark.parametrize("over,status,text", B_CASES, ids=[_id(c) for c in B_CASES])
def test_builder_rejection(over, status, text):
    got, msg = _call(BUILD, B_ORDER, B_VALID, over)
    assert (got, msg) == (status, f"{BUILD}: {text}" if text else "")


# -- which entry point spmm_csr takes -----------------------------------------------------------
class _Stop(Exception):
    pass


class _Lib:
    """Stands for libhgd: records the hop entry point spmm_csr calls, then stops the call."""

    def __init__(self, real):
        self._real = real
        self.called = []

    def __getattr__(self, name):
        if name.startswith("hgd_spmm") and "workspace" not in name and not name.endswith(
                ("_for", "_for_dt", "_fits")):
            def hop(*a):
                self.called.append((name, a))
                raise _Stop
            return hop
        if name == "hgd_gather32":  # (the weighted hops' reordered copy of val: not launched)
            return lambda *a: 0
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


def test_only_the_block_ordered_hop_with_a_source_scale_runs_packed(monkeypatch):
    """With three blocks, the order and packing forced: the fp32 hop over all rows whose caller
    states the source scale is hgd_spmm_blocked_packed, with the cached entries, dictionary and
    default bits; without the statement, with a row range, a bf16 side, a mask, a fused epilogue
    or no blocks it is the entry point it was, reading val."""
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "1")
    monkeypatch.setenv("HGD_SPMM_PACKED", "1")
    R, C, d = 40, 30, 8
    out = torch.zeros(R, d).as_subclass(_FakeCuda)

    def X(dtype=torch.float32):
        return torch.zeros(C, d, dtype=dtype).as_subclass(_FakeCuda)

    csr = _csr(R, C, 200)
    val, scale = torch.ones(200), torch.ones(C)
    ent, wdict, n_dict = _prime(csr, 3, scale, 5)

    def taken(csr=csr, x=None, **kw):
        return _hop_taken(monkeypatch, csr, X() if x is None else x, **kw)[0]

    name, a = _hop_taken(monkeypatch, csr, X(), out=out, val=val, src_scale=scale)
    assert name == "hgd_spmm_blocked_packed"
    assert a[1:5] == (ent.data_ptr(), wdict.data_ptr(), n_dict, BITS) and a[16] == 3
    assert not csr._blk_ord_vals  # the ordered copy of the weights was never built
    assert taken(out=out, src_scale=scale) == "hgd_spmm_blocked_packed"  # (val is not needed)
    assert taken(out=out, val=val) == "hgd_spmm_blocked_ordered"
    assert taken(out=out) == "hgd_spmm_blocked_ordered"
    assert taken(out=out, val=val, src_scale=scale, row_begin=1) == "hgd_spmm_blocked"
    assert taken(out=out, val=val, src_scale=scale, row_end=R - 1) == "hgd_spmm_blocked"
    out16 = torch.zeros(R, d, dtype=torch.bfloat16).as_subclass(_FakeCuda)
    assert taken(x=X(torch.bfloat16), out=out16, val=val, src_scale=scale) == "hgd_spmm_blocked_dt"
    assert taken(out=out16, val=val, src_scale=scale) == "hgd_spmm_blocked_dt"
    assert taken(out=out, val=val, src_scale=scale, ex=nat.RowEpilogue()) == "hgd_spmm_fused"
    assert taken(out=out, val=val, src_scale=scale, blocks=0) == "hgd_spmm"
    masked = _csr(R, C, 200)
    masked.mask, masked.keep = torch.ones(200, dtype=torch.uint8), 0.5
    assert taken(csr=masked, out=out, val=val, src_scale=scale) == "hgd_spmm_masked"
    monkeypatch.setenv("HGD_SPMM_PACKED", "0")
    assert taken(out=out, val=val, src_scale=scale) == "hgd_spmm_blocked_ordered"
    monkeypatch.delenv("HGD_SPMM_PACKED")  # the rule: forced blocks of 10 source rows are not packed
    assert taken(out=out, val=val, src_scale=scale) == "hgd_spmm_blocked_ordered"
    monkeypatch.setenv("HGD_SPMM_PACKED", "1")
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "0")
    assert taken(out=out, val=val, src_scale=scale) == "hgd_spmm_blocked"


def test_a_source_scale_without_val_is_an_error_off_the_packed_path(monkeypatch):
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    monkeypatch.setenv("HGD_SPMM_BLOCK_ORDER", "1")
    monkeypatch.setenv("HGD_SPMM_PACKED", "0")
    R, C, d = 40, 30, 8
    out = torch.zeros(R, d).as_subclass(_FakeCuda)
    x = torch.zeros(C, d).as_subclass(_FakeCuda)
    csr, scale = _csr(R, C, 200), torch.ones(C)
    monkeypatch.setattr(incidence, "_stream", lambda dev: None)
    with pytest.raises(ValueError, match="src_scale without val"):
        incidence.spmm_csr(csr, x, out=out, src_scale=scale)
    monkeypatch.setenv("HGD_SPMM_PACKED", "1")
    with pytest.raises(ValueError, match="src_scale without val"):
        incidence.spmm_csr(csr, x, out=out, src_scale=scale, row_begin=1)
    for bad in (torch.ones(C + 1), torch.ones(C, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"src_scale must be float32 \[n_cols\]"):
            incidence.spmm_csr(csr, x, out=out, val=torch.ones(200), src_scale=bad, blocks=0)


def test_the_two_hop_states_the_scale_of_a_binary_incidence_only():
    from hypergraph_diffusion_for_recommendation_amd.incidence import Incidence
    inc = Incidence.__new__(Incidence)
    inc.val = inc.val_t = None
    scale = torch.ones(3)
    inc.scale = lambda side, kind: (side, kind, scale) if kind else None
    assert inc.edge_src_scale("csc", "sym") == ("row", "sym", scale)
    assert inc.edge_src_scale("csr", "mean") == ("col", "mean", scale)
    assert inc.edge_src_scale("csc", None) is None
    inc.val = inc.val_t = torch.ones(5)  # values of its own folded into the weights: no statement
    assert inc.edge_src_scale("csc", "sym") is None and inc.edge_src_scale("csr", "sym") is None


def test_packed_implementation_bytes():
    from hypergraph_diffusion_for_recommendation_amd import profiling
    nnz, R, d, P_ = 1000, 100, 64, 4
    ordered = profiling.impl_bytes(nnz, R, d, True, True, P_, block_ordered=True)
    assert profiling.impl_bytes(nnz, R, d, True, True, P_, block_ordered=True,
                                packed=True) == ordered - 4 * nnz
    assert profiling.impl_bytes(nnz, R, d, True, True, P_, block_ordered=True,
                                packed=False) == ordered
    # an unweighted hop has no weight stream to take out, and the keyword counts nothing on a hop
    # that is not block-ordered; hop_bytes has no such term
    unweighted = profiling.impl_bytes(nnz, R, d, False, True, P_, block_ordered=True)
    assert profiling.impl_bytes(nnz, R, d, False, True, P_, block_ordered=True,
                                packed=True) == unweighted
    blocked = profiling.impl_bytes(nnz, R, d, True, True, P_)
    assert profiling.impl_bytes(nnz, R, d, True, True, P_, packed=True) == blocked
    plain = profiling.impl_bytes(nnz, R, d, True, True)
    assert profiling.impl_bytes(nnz, R, d, True, True, packed=True) == plain
    assert profiling.hop_bytes(nnz, R, d) == nnz * (4 + 4 * d) + R * (4 * d + 4) + (R + 1) * 4
