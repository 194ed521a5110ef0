"""The hop over bfloat16 tables (hgd_spmm_dt / hgd_spmm_masked_dt, HIP, gfx950).

Reference and bound: the inputs are rounded to bf16 on the CPU and the float64 oracle runs on the
rounded values. The kernel widens a bf16 element exactly and accumulates in fp32, so
  * an fp32 output obeys the suite's fp32 bound unchanged: |got - ref| <= 1e-5·Σ|terms|
    (tests/_util.py);
  * a bf16 output needs no tolerance: it is, bit for bit, the fp32 output of the same call
    rounded by torch (round to nearest even) — the same arithmetic, one rounding.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests._util import assert_close, dispatch_graph, random_coo

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _build(rows, cols, vals, shape, dev, **kw):
    from hypergraph_diffusion_for_recommendation_amd import Incidence
    idx = torch.from_numpy(np.stack([rows, cols]))
    v = None if vals is None else torch.from_numpy(vals.astype(np.float32))
    return Incidence.from_coo(idx, v, shape, device=dev, **kw)


def _bf16_table(rng, shape, dev):
    """A bf16 device table (finite values) and its exact float64 image for the oracle."""
    X = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).bfloat16()
    return X.to(dev), X.float().numpy().astype(np.float64)


def _both(csr, X, **kw):
    """The same hop with an fp32 and a bf16 output; asserts the bf16 one is the fp32 one rounded
    by torch, bit for bit, and returns the fp32 one."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    Y32 = spmm_csr(csr, X, out_dtype=F32, **kw)
    Y16 = spmm_csr(csr, X, out_dtype=BF16, **kw)
    assert Y32.dtype == F32 and Y16.dtype == BF16 and Y16.shape == Y32.shape
    assert torch.isfinite(Y32).all()
    assert torch.equal(Y16, Y32.to(BF16)), "the bf16 output is not the rounded fp32 output"
    return Y32


@pytest.mark.parametrize("d", [1, 3, 4, 8, 12, 16, 24, 64, 72, 128, 256, 320])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_bf16_spmm_dims(dev, d, weighted, scaled):
    """The scalar path (d % 8 != 0), the d % 8 edge (24, 72: a group wider than the row), one pass
    and several 128-column passes (256, 320: the last one narrower)."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    rng = np.random.default_rng(d * 7 + weighted + 2 * scaled)
    R, C = 173, 129
    r, c = random_coo(rng, R, C, 2500)
    vals = rng.standard_normal(len(r)).astype(np.float32) if weighted else None
    inc = _build(r, c, vals, (R, C), dev)
    X, Xr = _bf16_table(rng, (C, d), dev)
    scale = rng.random(R).astype(np.float32) if scaled else None
    s = None if scale is None else torch.from_numpy(scale).to(dev)
    Y32 = _both(inc.csr, X, val=inc.val, row_scale=s)
    rowptr, col, v, _ = O.csr_from_coo(r, c, R, vals)
    ref = O.spmm_csr(rowptr, col, Xr, v, scale)
    mag = O.spmm_csr(rowptr, col, Xr, v, scale, absolute=True)
    assert_close(Y32.cpu().numpy(), ref, mag, what=f"bf16→f32 d={d}")
    Y = spmm_csr(inc.csr, X, val=inc.val, row_scale=s)  # the default: X's dtype
    assert Y.dtype == BF16 and torch.equal(Y, Y32.to(BF16))


@pytest.mark.parametrize("d", [8, 64])
def test_f32_table_bf16_output(dev, d):
    """f32→bf16: bitwise hgd_spmm's output rounded by torch."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    rng = np.random.default_rng(70 + d)
    R, C = 173, 129
    r, c = random_coo(rng, R, C, 2500)
    vals = rng.standard_normal(len(r)).astype(np.float32)
    inc = _build(r, c, vals, (R, C), dev)
    X = torch.from_numpy(rng.standard_normal((C, d)).astype(np.float32)).to(dev)
    s = torch.from_numpy(rng.random(R).astype(np.float32)).to(dev)
    Y32 = spmm_csr(inc.csr, X, val=inc.val, row_scale=s)
    assert Y32.dtype == F32
    Y16 = spmm_csr(inc.csr, X, val=inc.val, row_scale=s, out_dtype=BF16)
    assert Y16.dtype == BF16 and torch.equal(Y16, Y32.to(BF16))
    out = torch.empty((R, d), dtype=BF16, device=dev)
    assert spmm_csr(inc.csr, X, val=inc.val, row_scale=s, out=out) is out
    assert torch.equal(out, Y16)


@pytest.mark.parametrize("d", [8, 64, 128])
def test_bf16_transpose_hop(dev, d):
    rng = np.random.default_rng(11 + d)
    R, C = 300, 77
    r, c = random_coo(rng, R, C, 4000)
    vals = rng.random(len(r)).astype(np.float32)
    inc = _build(r, c, vals, (R, C), dev)
    X, Xr = _bf16_table(rng, (R, d), dev)
    Y32 = _both(inc.csc, X, val=inc.val_t)
    ref = O.spmm_coo(c, r, vals, C, Xr)
    mag = O.spmm_coo(c, r, np.abs(vals), C, np.abs(Xr))
    assert_close(Y32.cpu().numpy(), ref, mag, what="bf16 Aᵀ·X")


@pytest.mark.parametrize("d", [8, 64, 256, 7])
@pytest.mark.parametrize("epi", [None, "leaky_relu", "relu"])
def test_bf16_split_rows_and_epilogue(dev, d, epi):
    """Long rows through the chunk split (threshold 16, chunk 8: fp32 partials, the fix-up kernel)
    with the fused activation, both output dtypes."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    rng = np.random.default_rng(5 + d)
    R, C = 64, 500
    degs = np.array([0, 1, 15, 16, 17, 24, 400, 3] + list(rng.integers(0, 40, R - 8)))
    rows = np.repeat(np.arange(R), degs)
    cols = np.concatenate([rng.choice(C, size=k, replace=False) for k in degs])
    vals = rng.standard_normal(len(rows)).astype(np.float32)
    inc = _build(rows, cols, vals, (R, C), dev, split_threshold=16, split_chunk=8)
    assert inc.csr.n_heavy > 0
    X, Xr = _bf16_table(rng, (C, d), dev)
    scale = rng.random(R).astype(np.float32)
    code = {None: nat.EPI_NONE, "leaky_relu": nat.EPI_LEAKY_RELU, "relu": nat.EPI_RELU}[epi]
    Y32 = _both(inc.csr, X, val=inc.val, row_scale=torch.from_numpy(scale).to(dev),
                epilogue=code, slope=0.2)
    rowptr, col, v, _ = O.csr_from_coo(rows, cols, R, vals)
    ref = O.spmm_csr(rowptr, col, Xr, v, scale, epi=epi, slope=0.2)
    mag = O.spmm_csr(rowptr, col, Xr, v, scale, absolute=True)
    assert_close(Y32.cpu().numpy(), ref, mag, what=f"bf16 split d={d} epi={epi}")


@pytest.mark.parametrize("d", [64, 128, 320, 32])
def test_bf16_segmented_kernel(dev, d):
    """The segmented short-row walk over a bf16 table: against the oracle and bitwise the row
    kernel. At d = 32 a group is 4 lanes: the segmented plan falls back to the row kernel."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    rng = np.random.default_rng(31 + d)
    R, C = 1037, 211
    degs = rng.integers(0, 14, R)
    degs[::17] = 0
    degs[5] = 40
    degs[6] = 17
    rows = np.repeat(np.arange(R), degs)
    cols = rng.integers(0, C, len(rows))
    vals = rng.standard_normal(len(rows)).astype(np.float32)
    inc = _build(rows, cols, vals, (R, C), dev)
    inc.csr.configure_kernel(segmented=True)
    assert inc.csr.segmented
    X, Xr = _bf16_table(rng, (C, d), dev)
    scale = rng.random(R).astype(np.float32)
    kw = dict(val=inc.val, row_scale=torch.from_numpy(scale).to(dev),
              epilogue=nat.EPI_LEAKY_RELU, slope=0.1)
    Y32 = _both(inc.csr, X, **kw)
    rowptr, col, v, _ = O.csr_from_coo(rows, cols, R, vals)
    ref = O.spmm_csr(rowptr, col, Xr, v, scale, epi="leaky_relu", slope=0.1)
    mag = O.spmm_csr(rowptr, col, Xr, v, scale, absolute=True)
    assert_close(Y32.cpu().numpy(), ref, mag, what=f"bf16 segmented d={d}")
    inc.csr.configure_kernel(segmented=False)
    assert not inc.csr.segmented
    assert torch.equal(_both(inc.csr, X, **kw), Y32)  # same per-row edge order → the same bits


@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("keep", [0.5, 0.7])
def test_bf16_masked_view(dev, d, keep):
    """The edge-dropped view (hgd_spmm_masked_dt) in every HGD_TUNE_MASK_PAIR mode: the same bits,
    the bits of the bf16 hop over the compacted structure (no row is split), and the oracle's
    sums over the kept edges weighted val / keep."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    rng = np.random.default_rng(int(keep * 10) + d)
    R, C = 2000, 1500
    r, c = random_coo(rng, R, C, 60_000)  # row-sorted: the COO order is the CSR order
    vals = (rng.random(len(r)) + 0.1).astype(np.float32)
    inc = _build(r, c, vals, (R, C), dev)
    assert inc.csr.n_heavy == 0 and inc.csc.n_heavy == 0
    m = rng.random(len(r)) < keep
    mask = torch.from_numpy(m.astype(np.uint8)).to(dev)
    X, Xr = _bf16_table(rng, (C, d), dev)
    Xt, Xtr = _bf16_table(rng, (R, d), dev)
    view = inc.masked(mask, keep)
    outs = {}
    try:
        for pair in (2, 1, 0):
            nat.check(lib.hgd_set_tuning(15, pair), "hgd_set_tuning")
            outs[pair] = (_both(view.csr, X, val=view.val), _both(view.csc, Xt, val=view.val_t))
    finally:
        nat.check(lib.hgd_set_tuning(15, 2), "hgd_set_tuning")
    for pair in (1, 0):
        assert torch.equal(outs[2][0], outs[pair][0]) and torch.equal(outs[2][1], outs[pair][1])
    child = view.materialize()
    assert torch.equal(outs[2][0], _both(child.csr, X, val=child.val))
    assert torch.equal(outs[2][1], _both(child.csc, Xt, val=child.val_t))
    kv = vals[m] / np.float32(keep)  # vals[mask] / keepRate in fp32, as the dropped COO's values
    rk, ck = r[m], c[m]
    assert_close(outs[2][0].cpu().numpy(), O.spmm_coo(rk, ck, kv, R, Xr),
                 O.spmm_coo(rk, ck, kv, R, np.abs(Xr)), what="bf16 masked A·X")
    assert_close(outs[2][1].cpu().numpy(), O.spmm_coo(ck, rk, kv, C, Xtr),
                 O.spmm_coo(ck, rk, kv, C, np.abs(Xtr)), what="bf16 masked Aᵀ·X")


def test_bf16_row_range_and_empty(dev):
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    rng = np.random.default_rng(3)
    R, C, d = 100, 40, 64
    r, c = random_coo(rng, R, C, 600)
    inc = _build(r, c, None, (R, C), dev)
    X, Xr = _bf16_table(rng, (C, d), dev)
    out = torch.full((R, d), 7.0, dtype=BF16, device=dev)
    out32 = torch.full((R, d), 7.0, dtype=F32, device=dev)
    spmm_csr(inc.csr, X, out=out, row_begin=30, row_end=55)
    spmm_csr(inc.csr, X, out=out32, row_begin=30, row_end=55)
    for t in (out, out32):
        assert bool((t[:30] == 7.0).all()) and bool((t[55:] == 7.0).all())
    assert torch.equal(out[30:55], out32[30:55].to(BF16))
    rowptr, col, _, _ = O.csr_from_coo(r, c, R)
    ref = O.spmm_csr(rowptr, col, Xr)
    mag = O.spmm_csr(rowptr, col, Xr, absolute=True)
    assert_close(out32[30:55].cpu().numpy(), ref[30:55], mag[30:55], what="bf16 row range")
    # empty structure: all-zero output
    inc0 = _build(np.zeros(0, np.int64), np.zeros(0, np.int64), None, (5, 9), dev)
    for dt in (BF16, F32):
        Y0 = spmm_csr(inc0.csr, torch.ones(9, 16, dtype=BF16, device=dev), out_dtype=dt)
        assert Y0.shape == (5, 16) and Y0.dtype == dt and float(Y0.float().abs().sum()) == 0.0


def test_bf16_unaligned_view(dev):
    """A column slice starting at an odd element of a wider bf16 tensor (2-byte aligned rows, a
    row stride that is no multiple of 8) takes the scalar path and still matches."""
    rng = np.random.default_rng(9)
    R, C = 50, 60
    r, c = random_coo(rng, R, C, 700)
    inc = _build(r, c, None, (R, C), dev)
    big, bigr = _bf16_table(rng, (C, 70), dev)
    X, Xr = big[:, 1:65], bigr[:, 1:65]
    assert X.data_ptr() % 4 == 2 and X.stride(0) == 70
    Y32 = _both(inc.csr, X)
    rowptr, col, _, _ = O.csr_from_coo(r, c, R)
    assert_close(Y32.cpu().numpy(), O.spmm_csr(rowptr, col, Xr),
                 O.spmm_csr(rowptr, col, Xr, absolute=True), what="bf16 unaligned")


def test_bf16_deterministic(dev):
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    rng = np.random.default_rng(21)
    R, C, d = 2000, 300, 64
    r, c = random_coo(rng, R, C, 60000)
    inc = _build(r, c, rng.random(len(r)).astype(np.float32), (R, C), dev, split_threshold=64,
                 split_chunk=16)
    assert inc.csc.n_heavy > 0  # split rows present
    X, _ = _bf16_table(rng, (C, d), dev)
    Xt, _ = _bf16_table(rng, (R, d), dev)
    for csr, T, v in ((inc.csr, X, inc.val), (inc.csc, Xt, inc.val_t)):
        Y1 = spmm_csr(csr, T, val=v)
        Y2 = spmm_csr(csr, T, val=v)
        assert Y1.dtype == BF16 and torch.equal(Y1, Y2)


def test_bf16_rejections(dev):
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    from hypergraph_diffusion_for_recommendation_amd.functional import two_hop_fused
    inc = _build(np.array([0, 1]), np.array([1, 0]), None, (2, 2), dev)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError):
            spmm_csr(inc.csr, torch.ones(2, 8, device=dev, dtype=dt))
        with pytest.raises(TypeError):
            spmm_csr(inc.csr, torch.ones(2, 8, device=dev), out_dtype=dt)
    ex = nat.RowEpilogue(act=nat.EPI_NONE, out_scale=1.0)
    with pytest.raises(TypeError, match="fused row epilogue"):
        spmm_csr(inc.csr, torch.ones(2, 8, device=dev, dtype=BF16), ex=ex)
    with pytest.raises(TypeError, match="fused row epilogue"):
        spmm_csr(inc.csr, torch.ones(2, 8, device=dev), ex=ex, out_dtype=BF16)
    with pytest.raises(TypeError):
        two_hop_fused(inc, torch.ones(2, 8, device=dev, dtype=BF16))
    with pytest.raises(TypeError):
        two_hop_fused(inc, torch.ones(2, 8, device=dev, dtype=BF16), epilogue="leaky_relu",
                      slope=-0.5)  # the unfused form of the same operator rejects it too


def _raw_hop(csr, X, val, scale, dt_codes):
    """hgd_spmm (dt_codes None) or hgd_spmm_dt straight through the C ABI, fp32 in and out."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import _stream, _ws
    lib = nat.load()
    d = X.shape[1]
    plan = ctypes.byref(csr.plan)
    wsb = lib.hgd_spmm_workspace_size(plan, d)
    ws = _ws(wsb, X.device) if wsb else None
    Y = torch.full((csr.n_rows, d), float("nan"), device=X.device)
    head = (csr.rowptr.data_ptr(), csr.col.data_ptr(), nat.ptr(val), nat.ptr(scale), csr.n_rows,
            csr.n_cols, 0, csr.n_rows)
    tail = (d, 0, 0.0, plan, nat.ptr(ws), wsb, _stream(X.device))
    if dt_codes is None:
        nat.check(lib.hgd_spmm(*head, X.data_ptr(), X.stride(0), Y.data_ptr(), Y.stride(0),
                               *tail), "hgd_spmm")
    else:
        nat.check(lib.hgd_spmm_dt(*head, X.data_ptr(), dt_codes[0], X.stride(0), Y.data_ptr(),
                                  dt_codes[1], Y.stride(0), *tail), "hgd_spmm_dt")
    return Y


@pytest.mark.parametrize("d", [8, 64, 7])
@pytest.mark.parametrize("split", [False, True])
def test_dt_entry_with_f32_codes_is_bitwise_hgd_spmm(dev, d, split):
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    rng = np.random.default_rng(400 + d + split)
    R, C = 173, 129
    r, c = random_coo(rng, R, C, 2500)
    vals = rng.standard_normal(len(r)).astype(np.float32)
    kw = dict(split_threshold=12, split_chunk=8) if split else {}
    inc = _build(r, c, vals, (R, C), dev, **kw)
    assert (inc.csr.n_heavy > 0) == split
    X = torch.from_numpy(rng.standard_normal((C, d)).astype(np.float32)).to(dev)
    s = torch.from_numpy(rng.random(R).astype(np.float32)).to(dev)
    a = _raw_hop(inc.csr, X, inc.val, s, None)
    b = _raw_hop(inc.csr, X, inc.val, s, (nat.DT_F32, nat.DT_F32))
    assert not a.isnan().any() and torch.equal(a, b)
    assert torch.equal(a, spmm_csr(inc.csr, X, val=inc.val, row_scale=s))
    assert torch.equal(a, spmm_csr(inc.csr, X, val=inc.val, row_scale=s, out_dtype=F32))


@pytest.mark.parametrize("d", [320, 136])
@pytest.mark.parametrize("y_dtype", [BF16, F32])
def test_bf16_pass_cols_is_bitwise_auto(dev, d, y_dtype):
    """HGD_TUNE_SPMM_PASS_COLS ∈ {64, 128, 256} against 0 (auto, 128 with a 16-bit side) over a
    bf16 table: column passes are independent, so the width of a pass changes no bit. d = 136 is
    aligned but no multiple of a pass. Rows are whole here: a split row's fix-up adds its chunk
    partials in an order that follows the groups per block, hence the pass width. The auto output
    obeys the file's bounds."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    lib = nat.load()
    rows, cols, vals = dispatch_graph(7)
    R, C = 300, 257
    inc = _build(rows, cols, vals, (R, C), dev, split_threshold=0)
    assert inc.csr.n_heavy == 0
    rng = np.random.default_rng(d)
    X, Xr = _bf16_table(rng, (C, d), dev)
    scale = rng.random(R).astype(np.float32)
    s = torch.from_numpy(scale).to(dev)

    def hop():
        Y = torch.full((R, d), float("nan"), dtype=y_dtype, device=dev)
        spmm_csr(inc.csr, X, val=inc.val, row_scale=s, out=Y)
        return Y

    try:
        nat.check(lib.hgd_set_tuning(3, 0), "hgd_set_tuning")
        base = hop()
        for pass_cols in (64, 128, 256):
            nat.check(lib.hgd_set_tuning(3, pass_cols), "hgd_set_tuning")
            assert torch.equal(hop(), base), (d, y_dtype, pass_cols)
    finally:
        nat.check(lib.hgd_set_tuning(3, 0), "hgd_set_tuning")
    Y32 = _both(inc.csr, X, val=inc.val, row_scale=s)
    assert torch.equal(base, Y32.to(y_dtype))
    rowptr, col, v, _ = O.csr_from_coo(rows, cols, R, vals)
    assert_close(Y32.cpu().numpy(), O.spmm_csr(rowptr, col, Xr, v, scale),
                 O.spmm_csr(rowptr, col, Xr, v, scale, absolute=True),
                 what=f"bf16 pass cols auto d={d}")


def test_bf16_hop_ignores_the_tuning_matrix(dev):
    """A bf16 hop at d = 64 runs U = 8 with the prefetch policy whatever HGD_TUNE_SPMM_UNROLL /
    HGD_TUNE_SPMM_POLICY say: bitwise its default-tuning output with unroll 16 and policy 1."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    rows, cols, vals = dispatch_graph(7)
    R, C, d = 300, 257, 64
    inc = _build(rows, cols, vals, (R, C), dev, split_threshold=16, split_chunk=8)
    X, _ = _bf16_table(np.random.default_rng(64), (C, d), dev)
    try:
        base = _both(inc.csr, X, val=inc.val)
        assert bool(base.abs().sum() > 0)
        nat.check(lib.hgd_set_tuning(1, 16), "hgd_set_tuning")
        nat.check(lib.hgd_set_tuning(2, 1), "hgd_set_tuning")
        assert torch.equal(_both(inc.csr, X, val=inc.val), base)
    finally:
        nat.check(lib.hgd_set_tuning(1, 8), "hgd_set_tuning")
        nat.check(lib.hgd_set_tuning(2, 8), "hgd_set_tuning")
