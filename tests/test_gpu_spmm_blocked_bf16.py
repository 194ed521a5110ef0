"""The source-blocked hop over bfloat16 tables (hgd_spmm_blocked_dt, HIP, gfx950).

Reference and bounds, as in tests/test_gpu_spmm_bf16.py: the inputs are rounded to bf16 on the
CPU and the float64 oracle runs on the rounded values. The kernel widens a bf16 element exactly
and sums in fp32, blockwise (a different association of the same terms, as the fp32 blocked hop),
so
  * an fp32 output obeys the suite's fp32 bound: |got - ref| <= 1e-5·Σ|terms| (tests/_util.py);
  * a bf16 output needs no tolerance: the blocks' running partial stays fp32 (in a scratch), so
    it is, bit for bit, the fp32 output of the same call rounded by torch — one rounding, not P.

The graph is the fp32 blocked tests' (tests/test_gpu_spmm.py): 2001 users × 613 items, about
30 k nonzeros, no split rows; the hop runs over its CSC (rows = items, sources = users).
"""
import functools
import gc

import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests._util import assert_close, random_coo

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
R, C = 2001, 613  # users (the gathered side), items (the rows of the CSC)
RB, RE = 11, 600  # the row range of the oracle cases
U_BF16 = 2.0 ** -9  # the constants of tests/test_gpu_two_hop_bf16.py's two-hop bound, restated
MARGIN = 2.0


def _rtol(k):
    """tests/test_gpu_two_hop_bf16.py's bound of a value that went through k bf16 stores."""
    return k * U_BF16 * MARGIN + 1e-5


def _build(rows, cols, vals, shape, dev, **kw):
    from hypergraph_diffusion_for_recommendation_amd import Incidence
    idx = torch.from_numpy(np.stack([rows, cols]))
    v = None if vals is None else torch.from_numpy(vals.astype(np.float32))
    return Incidence.from_coo(idx, v, shape, device=dev, **kw)


@pytest.fixture(scope="module")
def case(dev):
    """The structure, weights and row scale every one-hop test shares (never modified)."""
    rng = np.random.default_rng(4242)
    r, c = random_coo(rng, R, C, 30000)
    vals = rng.standard_normal(len(r)).astype(np.float32)
    inc = _build(r, c, vals, (R, C), dev, split_threshold=0)
    assert inc.csc.cols_ascending and inc.csc.n_heavy == 0 and not inc.csc.segmented
    q = rng.random(C).astype(np.float32)
    rowptr, col, v, _ = O.csr_from_coo(c, r, C, vals)
    return dict(r=r, c=c, vals=vals, inc=inc, q=q, qd=torch.from_numpy(q).to(dev),
                rowptr=rowptr, col=col, v=v)


@functools.lru_cache(maxsize=None)
def _table(d):
    """A bf16 table [R, d] (CPU) and its exact float64 image, one per width."""
    rng = np.random.default_rng(1000 + d)
    X = torch.from_numpy(rng.standard_normal((R, d)).astype(np.float32)).bfloat16()
    return X, X.float().numpy().astype(np.float64)


_REFS = {}


def _oracle(case, d, epi):
    """(ref, mag) of the hop at width d, computed once per (d, activation)."""
    got = _REFS.get((d, epi))
    if got is None:
        Xr = _table(d)[1]
        ref = O.spmm_csr(case["rowptr"], case["col"], Xr, case["v"], case["q"], epi=epi, slope=0.2)
        mag = O.spmm_csr(case["rowptr"], case["col"], Xr, case["v"], case["q"], absolute=True)
        got = _REFS[(d, epi)] = (ref, mag)
    return got


def _range_hop(case, X, y_dtype, code):
    """The hop over rows [RB, RE) into a NaN-filled output of y_dtype."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    inc = case["inc"]
    Y = torch.full((C, X.shape[1]), float("nan"), dtype=y_dtype, device=X.device)
    spmm_csr(inc.csc, X, val=inc.val_t, row_scale=case["qd"], out=Y, row_begin=RB, row_end=RE,
             epilogue=code, slope=0.2)
    assert bool(Y[:RB].isnan().all()) and bool(Y[RE:].isnan().all()), "rows outside the range"
    assert bool(torch.isfinite(Y[RB:RE]).all())
    return Y


def _raw_blocked(csc, X, val, scale, P, y_dtype, codes=None, epilogue=0, slope=0.0, Y=None):
    """hgd_spmm_blocked_dt (codes = (x, y) dtype codes; default: the tensors' own) straight
    through the C ABI over csc.col_blocks(P), every row."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import _HOP_DTYPES, _stream, _ws
    lib = nat.load()
    d = X.shape[1]
    if codes is None:
        codes = (_HOP_DTYPES[X.dtype], _HOP_DTYPES[y_dtype])
    start, bcol, _ = csc.col_blocks(P)
    bval = csc.blocked_values(P, val)
    if Y is None:
        Y = torch.full((csc.n_rows, d), float("nan"), dtype=y_dtype, device=X.device)
    wsb = lib.hgd_spmm_blocked_dt_workspace_size(csc.n_rows, d, codes[1], P)
    assert (wsb > 0) == (y_dtype == BF16 and P > 1)
    ws = _ws(wsb, X.device) if wsb else None
    nat.check(lib.hgd_spmm_blocked_dt(
        start.data_ptr(), bcol.data_ptr(), nat.ptr(bval), nat.ptr(scale), csc.n_rows, csc.n_cols,
        0, csc.n_rows, X.data_ptr(), codes[0], X.stride(0), Y.data_ptr(), codes[1], Y.stride(0),
        d, epilogue, slope, P, nat.ptr(ws), wsb, _stream(X.device)), "hgd_spmm_blocked_dt")
    return Y


@pytest.fixture(scope="module")
def sparse_case(dev):
    """The same shape with a third of the items empty and a third with one or two nonzeros:
    empty rows, rows living entirely in one block and rows with no nonzero in some block."""
    rng = np.random.default_rng(99)
    r, c = random_coo(rng, R, C, 9000)
    keep = (c % 3 == 0) | ((c % 3 == 2) & (r % 8 == 0))
    r, c = r[keep], c[keep]
    vals = rng.standard_normal(len(r)).astype(np.float32)
    inc = _build(r, c, vals, (R, C), dev, split_threshold=0)
    q = rng.random(C).astype(np.float32)
    rowptr, col, v, _ = O.csr_from_coo(c, r, C, vals)
    return dict(inc=inc, q=q, qd=torch.from_numpy(q).to(dev), rowptr=rowptr, col=col, v=v)


@pytest.mark.parametrize("d", [7, 8, 24, 64, 136, 256, 320])
@pytest.mark.parametrize("n_blocks", [2, 3, 5])
@pytest.mark.parametrize("epi", [None, "leaky_relu"])
def test_blocked_bf16_matches_the_oracle_and_rounds_once(dev, monkeypatch, case, d, n_blocks, epi):
    """hgd_spmm_blocked_dt through spmm_csr (forced by HGD_SPMM_BLOCKS) over a bf16 table: d = 7
    the scalar path, 24 a group wider than the row, 136 and 320 a last pass narrower than 128.
    The fp32 output within 1e-5·Σ|terms| of the float64 oracle; the bf16 output the fp32 one
    rounded by torch, bit for bit; rows outside the range untouched."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_blocks
    monkeypatch.setenv("HGD_SPMM_BLOCKS", str(n_blocks))
    assert spmm_blocks(case["inc"].csc, d, BF16) == n_blocks
    X = _table(d)[0].to(dev)
    code = {None: nat.EPI_NONE, "leaky_relu": nat.EPI_LEAKY_RELU}[epi]
    Y32 = _range_hop(case, X, F32, code)
    Y16 = _range_hop(case, X, BF16, code)
    ref, mag = _oracle(case, d, epi)
    got = Y32[RB:RE].cpu().numpy()
    print(f"d={d} P={n_blocks} epi={epi}: max rel err "
          f"{np.max(np.abs(got - ref[RB:RE]) / (mag[RB:RE] + 1e-30)):.3e}")
    assert_close(got, ref[RB:RE], mag[RB:RE], what=f"blocked bf16→f32 d={d} P={n_blocks} {epi}")
    assert torch.equal(Y16[RB:RE], Y32[RB:RE].to(BF16)), "the bf16 output is not the rounded fp32"


@pytest.mark.parametrize("d", [8, 64])
def test_blocked_f32_table_bf16_output(dev, monkeypatch, case, d):
    """f32 → bf16 in 3 blocks: bitwise hgd_spmm_blocked's output rounded by torch."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    inc = case["inc"]
    rng = np.random.default_rng(70 + d)
    X = torch.from_numpy(rng.standard_normal((R, d)).astype(np.float32)).to(dev)
    kw = dict(val=inc.val_t, row_scale=case["qd"], epilogue=1, slope=0.2)
    Y32 = spmm_csr(inc.csc, X, **kw)  # float32 in and out: hgd_spmm_blocked
    Y16 = spmm_csr(inc.csc, X, out_dtype=BF16, **kw)
    assert Y32.dtype == F32 and Y16.dtype == BF16
    assert torch.equal(Y16, Y32.to(BF16))
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "0")
    assert not torch.equal(spmm_csr(inc.csc, X, **kw), Y32)  # (it was blocked: other bits)


@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("n_blocks", [2, 5])
def test_blocked_bf16_empty_and_one_block_rows(dev, monkeypatch, sparse_case, d, n_blocks):
    """A structure with a third of its rows empty and most others in one or two blocks: every
    row is written (an empty row as zero), both output types, against the oracle."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    monkeypatch.setenv("HGD_SPMM_BLOCKS", str(n_blocks))
    sc = sparse_case
    inc = sc["inc"]
    deg = np.diff(sc["rowptr"])
    cnt = np.diff(inc.csc.col_blocks(n_blocks)[0].cpu().numpy()).reshape(n_blocks, C)
    assert (cnt.sum(axis=0) == deg).all()
    assert (deg == 0).sum() > C // 4                 # empty rows
    assert ((cnt > 0).sum(axis=0) == 1).sum() > 20   # rows living entirely in one block
    assert ((cnt == 0).any(axis=0) & (deg > 1)).any()  # longer rows missing a block
    X, Xr = _table(d)
    X = X.to(dev)
    out = {}
    for dt in (F32, BF16):
        Y = torch.full((C, d), float("nan"), dtype=dt, device=dev)
        spmm_csr(inc.csc, X, val=inc.val_t, row_scale=sc["qd"], out=Y)
        out[dt] = Y
    assert bool(torch.isfinite(out[F32]).all())
    assert bool((out[F32][torch.from_numpy(deg == 0).to(dev)] == 0).all())
    assert torch.equal(out[BF16], out[F32].to(BF16))
    ref = O.spmm_csr(sc["rowptr"], sc["col"], Xr, sc["v"], sc["q"])
    mag = O.spmm_csr(sc["rowptr"], sc["col"], Xr, sc["v"], sc["q"], absolute=True)
    assert_close(out[F32].cpu().numpy(), ref, mag, what=f"sparse blocked d={d} P={n_blocks}")


@pytest.mark.parametrize("d", [7, 64])
@pytest.mark.parametrize("pair", [(BF16, BF16), (BF16, F32), (F32, BF16)],
                         ids=["bf16_bf16", "bf16_f32", "f32_bf16"])
def test_one_block_is_bitwise_hgd_spmm_dt(dev, monkeypatch, case, d, pair):
    """hgd_spmm_blocked_dt with n_blocks = 1 walks [rowptr[r], rowptr[r+1]) exactly as
    hgd_spmm_dt (no workspace either)."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "0")  # the plain hop, whatever the environment says
    inc = case["inc"]
    X = _table(d)[0].to(dev)
    if pair[0] == F32:
        X = X.float() * 1.0009765625  # (no longer bf16 values)
    plain = spmm_csr(inc.csc, X, val=inc.val_t, row_scale=case["qd"], out_dtype=pair[1])
    one = _raw_blocked(inc.csc, X, inc.val_t, case["qd"], 1, pair[1])
    assert plain.dtype == pair[1] and not one.isnan().any() and torch.equal(one, plain)


def test_f32_codes_forward_to_hgd_spmm_blocked(dev, monkeypatch, case):
    """With HGD_DT_F32 / HGD_DT_F32 the entry point is hgd_spmm_blocked, bitwise, at P = 3."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    inc = case["inc"]
    for d in (7, 64):
        X = _table(d)[0].to(dev).float()
        ref = spmm_csr(inc.csc, X, val=inc.val_t, row_scale=case["qd"])  # hgd_spmm_blocked
        got = _raw_blocked(inc.csc, X, inc.val_t, case["qd"], 3, F32,
                           codes=(nat.DT_F32, nat.DT_F32))
        assert not got.isnan().any() and torch.equal(got, ref)


def test_spmm_csr_really_blocks_a_bf16_hop(dev, monkeypatch, case):
    """With HGD_SPMM_BLOCKS=3 spmm_csr over a bf16 table IS hgd_spmm_blocked_dt over
    col_blocks(3); ``blocks=0`` keeps the plain hgd_spmm_dt; a masked view and a structure
    with split rows are never blocked."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_blocks
    inc = case["inc"]
    d = 64
    X = _table(d)[0].to(dev)
    kw = dict(val=inc.val_t, row_scale=case["qd"])
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "0")
    plain = {dt: spmm_csr(inc.csc, X, out_dtype=dt, **kw) for dt in (F32, BF16)}
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    assert spmm_blocks(inc.csc, d, BF16) == 3 and spmm_blocks(inc.csr, d, BF16) == 0
    for dt in (F32, BF16):
        got = spmm_csr(inc.csc, X, out_dtype=dt, **kw)
        direct = _raw_blocked(inc.csc, X, inc.val_t, case["qd"], 3, dt)
        assert got.dtype == dt and torch.equal(got, direct)
        assert torch.equal(spmm_csr(inc.csc, X, out_dtype=dt, blocks=0, **kw), plain[dt])
    # blockwise partials are another association: the fp32 outputs differ somewhere
    assert not torch.equal(spmm_csr(inc.csc, X, out_dtype=F32, **kw), plain[F32])
    # a masked view: the masked kernel, bitwise what it gives with blocking off
    rng = np.random.default_rng(5)
    mask = torch.from_numpy((rng.random(inc.nnz) < 0.5).astype(np.uint8)).to(dev)
    view = inc.masked(mask, 0.5)
    assert spmm_blocks(view.csc, d, BF16) == 0
    m3 = spmm_csr(view.csc, X, val=view.val_t)
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "0")
    assert torch.equal(m3, spmm_csr(view.csc, X, val=view.val_t))
    # split rows (in either orientation) turn it off
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    split = _build(case["r"], case["c"], case["vals"], (R, C), dev, split_threshold=16,
                   split_chunk=8)
    assert split.csr.n_heavy > 0 and split.csc.n_heavy > 0
    assert spmm_blocks(split.csr, d, BF16) == 0 and spmm_blocks(split.csc, d, BF16) == 0
    Xi = _table(d)[0][:C].to(dev)
    s3 = spmm_csr(split.csr, Xi, val=split.val)
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "0")
    assert torch.equal(s3, spmm_csr(split.csr, Xi, val=split.val))


@pytest.fixture(scope="module")
def two_hop_case(dev):
    rng = np.random.default_rng(123)
    U, I, d = 3000, 400, 64
    r, c = random_coo(rng, U, I, 40000)
    inc = _build(r, c, None, (U, I), dev, split_threshold=0)
    E = rng.standard_normal((U, d)).astype(np.float32)
    dY = rng.standard_normal((U, d)).astype(np.float32)
    return dict(r=r, c=c, inc=inc, shape=(U, I), E=E, dY=dY)


def test_blocked_bf16_two_hop_fwd_bwd(dev, monkeypatch, two_hop_case):
    """hgconv2 over bf16 tables under fp32 master weights with the hops into items blocked
    (HGD_SPMM_BLOCKS=4): forward against the float64 two-hop of the rounded table (M goes through
    one bf16 store), the fp32 gradient against the oracle's (two stores) and against the same
    call's unblocked gradient, all within tests/test_gpu_two_hop_bf16.py's bound. The bf16 → bf16
    form: its output is the fp32-output form's rounded once — to bf16's half-ulp, not asserted
    bitwise (only the one-hop identity is)."""
    from hypergraph_diffusion_for_recommendation_amd import hgconv2
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_blocks
    t = two_hop_case
    inc, shape, r, c = t["inc"], t["shape"], t["r"], t["c"]
    kinds = dict(P="sym", Q="mean", R="sym")
    dY = torch.from_numpy(t["dY"]).to(dev)

    def run():
        E32 = torch.from_numpy(t["E"]).to(dev).requires_grad_(True)
        Y = hgconv2(inc, E32.bfloat16(), out_dtype=F32)
        Y.backward(dY)
        return Y.detach(), E32.grad

    monkeypatch.setenv("HGD_SPMM_BLOCKS", "4")
    assert spmm_blocks(inc.csc, 64, BF16) == 4 and spmm_blocks(inc.csr, 64, BF16) == 0
    Y, g = run()
    assert Y.dtype == F32 and g is not None and g.dtype == F32
    Y16 = hgconv2(inc, torch.from_numpy(t["E"]).to(dev).bfloat16())
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "0")
    _, g0 = run()
    Xr = torch.from_numpy(t["E"]).bfloat16().float().numpy().astype(np.float64)
    ref = O.two_hop(r, c, None, shape, Xr, **kinds)
    mag = O.two_hop(r, c, None, shape, np.abs(Xr), **kinds)
    assert_close(Y.cpu().numpy(), ref, mag, rtol=_rtol(1), what="blocked bf16 hgconv2 Y")
    dYr = t["dY"].astype(np.float64)
    dref = O.two_hop_backward(r, c, None, shape, None, dYr, **kinds)
    dmag = O.two_hop_backward(r, c, None, shape, None, np.abs(dYr), **kinds)
    assert_close(g.cpu().numpy(), dref, dmag, rtol=_rtol(2), what="blocked E32.grad")
    assert_close(g.cpu().numpy(), g0.cpu().numpy(), dmag, rtol=_rtol(2),
                 what="blocked against unblocked E32.grad")
    # bf16 → bf16: one more rounding of the same sums. bf16 keeps 8 significant bits, so the
    # values around x in [2^e, 2^(e+1)) are 2^(e-7) apart and round-to-nearest moves x by at most
    # half of that: |x − rn(x)| <= 2^(e-8) <= 2^-8·|x|
    assert Y16.dtype == BF16
    y32 = Y.cpu().numpy().astype(np.float64)
    assert_close(Y16.float().cpu().numpy(), y32, np.abs(y32) + 1e-30, rtol=2.0 ** -8,
                 what="bf16→bf16 against the fp32-output form")


def test_blocked_bf16_two_hop_replays_in_a_hip_graph(dev, monkeypatch, two_hop_case):
    """The blocked bf16 two-hop, fwd + bwd under fp32 master weights, its all-bf16 form and the
    one-hop bf16 → f32 hop captured in one HIP graph after eager warm-up (which builds the
    block-major copy and the blocked weights): three replays, each bitwise the eager step — the
    entry point neither allocates nor synchronises."""
    from hypergraph_diffusion_for_recommendation_amd import hgconv2, spmm_csr
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "4")
    t = two_hop_case
    inc = t["inc"]
    E32 = torch.from_numpy(t["E"]).to(dev).requires_grad_(True)
    dY = torch.from_numpy(t["dY"]).to(dev)

    def step():
        Eb = E32.bfloat16()
        Y = hgconv2(inc, Eb, out_dtype=F32)
        (g,) = torch.autograd.grad(Y, E32, dY)
        with torch.no_grad():
            Yb = hgconv2(inc, Eb.detach())
            M32 = spmm_csr(inc.csc, Eb.detach(), val=inc.val_t, out_dtype=F32)
        return Y, g, Yb, M32

    eager = [x.detach() for x in step()]  # an eager output holding its graph breaks the capture
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    # thread-local: autograd's device thread runs the backward during the capture
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        captured = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize(dev)
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)


def test_blocked_bf16_is_deterministic(dev, monkeypatch, case):
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "5")
    inc = case["inc"]
    X = _table(64)[0].to(dev)
    for dt in (F32, BF16):
        Y1 = spmm_csr(inc.csc, X, val=inc.val_t, row_scale=case["qd"], out_dtype=dt)
        Y2 = spmm_csr(inc.csc, X, val=inc.val_t, row_scale=case["qd"], out_dtype=dt)
        assert Y1.dtype == dt and torch.equal(Y1, Y2)
