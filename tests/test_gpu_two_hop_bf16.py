"""hgconv2 / mean2hop over a bfloat16 table: forward, backward, fp32 master weights and the
HIP-graph replay.

Two statements per result:
  * it is, bit for bit, the composition of the one-hop calls of tests/test_gpu_spmm_bf16.py (the
    same spmm_csr calls with the same weights, row scales and output dtypes), and
  * it is within a derived bound of the float64 oracle run on the bf16-rounded inputs: a value that
    passes through k bf16 stores obeys |got - ref| <= (k·2^-9·m + 1e-5)·Σ|terms|, where 2^-9 is
    bf16's unit round-off, m = 2 a margin for rounding computed values rather than exact ones and
    1e-5 the suite's fp32 bound. k = 1 for an fp32 Y (M is stored in bf16), 2 for a bf16 Y; 2 / 3
    likewise for dX.
"""
import gc

import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests._util import assert_close, random_coo

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
U_BF16 = 2.0 ** -9
MARGIN = 2.0
SHAPE = (2001, 613)
OPS = {"hgconv2": dict(P="sym", Q="mean", R="sym"), "mean2hop": dict(P="mean", Q="mean", R=None)}


def _rtol(k):
    return k * U_BF16 * MARGIN + 1e-5


@pytest.fixture(scope="module")
def graph(dev):
    """One structure shared by the cases (never modified)."""
    from hypergraph_diffusion_for_recommendation_amd import Incidence
    rng = np.random.default_rng(2024)
    r, c = random_coo(rng, SHAPE[0], SHAPE[1], 20_400)
    inc = Incidence.from_coo(torch.from_numpy(np.stack([r, c])), None, SHAPE, device=dev)
    return r, c, inc


def _rounded(rng, shape, dev, dtype):
    """A device tensor of ``dtype`` and its exact float64 image."""
    t = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    if dtype == BF16:
        t = t.bfloat16()
    return t.to(dev), t.float().numpy().astype(np.float64)


def _one_hop_composition(inc, X, dY, P, Q, R, y_dtype):
    """The two-hop and its backward written as the four spmm_csr calls."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    q = inc.scale("col", Q)
    M = spmm_csr(inc.csc, X, val=inc.edge_values("csc", R), row_scale=q)
    assert M.dtype == X.dtype
    Y = spmm_csr(inc.csr, M, val=inc.val, row_scale=inc.scale("row", P), out_dtype=y_dtype)
    dM = spmm_csr(inc.csc, dY, val=inc.edge_values("csc", P), row_scale=q, out_dtype=X.dtype)
    dX = spmm_csr(inc.csr, dM, val=inc.val, row_scale=inc.scale("row", R), out_dtype=X.dtype)
    return M, Y, dX


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("op", ["hgconv2", "mean2hop"])
@pytest.mark.parametrize("y_dtype", [BF16, F32], ids=["bf16_out", "f32_out"])
def test_bf16_two_hop_forward_backward(dev, graph, d, op, y_dtype):
    import hypergraph_diffusion_for_recommendation_amd as hgd
    r, c, inc = graph
    kinds = OPS[op]
    rng = np.random.default_rng(d + len(op) + (y_dtype == F32))
    X, Xr = _rounded(rng, (SHAPE[0], d), dev, BF16)
    dY, dYr = _rounded(rng, (SHAPE[0], d), dev, y_dtype)
    Xg = X.clone().requires_grad_(True)
    Y = getattr(hgd, op)(inc, Xg, out_dtype=None if y_dtype == BF16 else F32)
    (dX,) = torch.autograd.grad(Y, Xg, dY)
    assert Y.dtype == y_dtype and dX.dtype == BF16
    M, Yc, dXc = _one_hop_composition(inc, X, dY, y_dtype=y_dtype, **kinds)
    assert M.dtype == BF16
    assert torch.equal(Y.detach(), Yc) and torch.equal(dX, dXc)
    ky = 2 if y_dtype == BF16 else 1
    ref = O.two_hop(r, c, None, SHAPE, Xr, **kinds)
    mag = O.two_hop(r, c, None, SHAPE, np.abs(Xr), **kinds)
    assert_close(Y.detach().float().cpu().numpy(), ref, mag, rtol=_rtol(ky), what=f"{op} Y")
    # M alone: one bf16 store
    Rs = O._scale(r, np.ones(len(r)), SHAPE[0], kinds["R"])
    Qs = O._scale(c, np.ones(len(r)), SHAPE[1], kinds["Q"])
    Mref = O.spmm_coo(c, r, None, SHAPE[1], Xr * Rs[:, None]) * Qs[:, None]
    Mmag = O.spmm_coo(c, r, None, SHAPE[1], np.abs(Xr) * Rs[:, None]) * Qs[:, None]
    assert_close(M.float().cpu().numpy(), Mref, Mmag, rtol=_rtol(1), what=f"{op} M")
    dref = O.two_hop_backward(r, c, None, SHAPE, None, dYr, **kinds)
    dmag = O.two_hop_backward(r, c, None, SHAPE, None, np.abs(dYr), **kinds)
    assert_close(dX.float().cpu().numpy(), dref, dmag, rtol=_rtol(ky + 1), what=f"{op} dX")


@pytest.mark.parametrize("d", [16, 64])
def test_fp32_master_weights_get_an_fp32_gradient(dev, graph, d):
    """``hgconv2(inc, E32.bfloat16(), out_dtype=torch.float32)``: bf16 hops under fp32 master
    weights — autograd's cast hands E32 an fp32 gradient."""
    from hypergraph_diffusion_for_recommendation_amd import hgconv2
    r, c, inc = graph
    kinds = OPS["hgconv2"]
    rng = np.random.default_rng(900 + d)
    E32 = torch.from_numpy(rng.standard_normal((SHAPE[0], d)).astype(np.float32)).to(dev)
    E32.requires_grad_(True)
    dY, dYr = _rounded(rng, (SHAPE[0], d), dev, F32)
    Y = hgconv2(inc, E32.bfloat16(), out_dtype=F32)
    assert Y.dtype == F32
    Y.backward(dY)
    assert E32.grad is not None and E32.grad.dtype == F32
    Xr = E32.detach().bfloat16().float().cpu().numpy().astype(np.float64)
    ref = O.two_hop(r, c, None, SHAPE, Xr, **kinds)
    mag = O.two_hop(r, c, None, SHAPE, np.abs(Xr), **kinds)
    assert_close(Y.detach().cpu().numpy(), ref, mag, rtol=_rtol(1), what="hgconv2 Y (f32 out)")
    dref = O.two_hop_backward(r, c, None, SHAPE, None, dYr, **kinds)
    dmag = O.two_hop_backward(r, c, None, SHAPE, None, np.abs(dYr), **kinds)
    assert_close(E32.grad.cpu().numpy(), dref, dmag, rtol=_rtol(2), what="E32.grad")
    _, _, dXc = _one_hop_composition(inc, E32.detach().bfloat16(), dY, y_dtype=F32, **kinds)
    assert torch.equal(E32.grad, dXc.float())


def test_bf16_spmm_autograd_and_epilogues(dev, graph):
    """functional.spmm (what layers.GCNLayer calls) with a bf16 table, and the two-hop's fused
    and un-fusable (slope < 0) activations against the one-hop composition."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd import spmm, spmm_csr, two_hop
    r, c, inc = graph
    rng = np.random.default_rng(77)
    d = 64
    X, _ = _rounded(rng, (SHAPE[1], d), dev, BF16)
    dY, _ = _rounded(rng, (SHAPE[0], d), dev, BF16)
    Xg = X.clone().requires_grad_(True)
    Y = spmm(inc, Xg)
    (dX,) = torch.autograd.grad(Y, Xg, dY)
    assert Y.dtype == BF16 and dX.dtype == BF16
    assert torch.equal(Y.detach(), spmm_csr(inc.csr, X, val=inc.val))
    assert torch.equal(dX, spmm_csr(inc.csc, dY, val=inc.val_t))
    Xu, _ = _rounded(rng, (SHAPE[0], d), dev, BF16)
    for slope in (0.2, -0.5):
        Xg = Xu.clone().requires_grad_(True)
        Y = two_hop(inc, Xg, P="mean", Q="mean", epilogue="leaky_relu", slope=slope)
        (dX,) = torch.autograd.grad(Y, Xg, dY)
        M = spmm_csr(inc.csc, Xu, row_scale=inc.scale("col", "mean"))
        p = inc.scale("row", "mean")
        if slope >= 0:
            Yc = spmm_csr(inc.csr, M, row_scale=p, epilogue=nat.EPI_LEAKY_RELU, slope=slope)
            pos = Yc > 0
        else:
            Z = spmm_csr(inc.csr, M, row_scale=p)
            pos = Z > 0
            Yc = torch.where(pos, Z, Z * slope)
        assert Y.dtype == BF16 and torch.equal(Y.detach(), Yc)
        dZ = torch.where(pos, dY, dY * slope)
        dM = spmm_csr(inc.csc, dZ, val=inc.edge_values("csc", "mean"),
                      row_scale=inc.scale("col", "mean"))
        assert torch.equal(dX, spmm_csr(inc.csr, dM))


def test_bf16_two_hop_replays_in_a_hip_graph(dev, graph):
    """One bf16 hgconv2 forward + backward captured in a HIP graph after an eager warm-up: every
    replay is bitwise the eager step, and the captured step builds nothing new (the structure's
    scales, folded weights and workspace sizes all exist after the warm-up)."""
    from hypergraph_diffusion_for_recommendation_amd import hgconv2
    _, _, inc = graph
    rng = np.random.default_rng(321)
    d = 64
    X, _ = _rounded(rng, (SHAPE[0], d), dev, BF16)
    dY, _ = _rounded(rng, (SHAPE[0], d), dev, BF16)
    X.requires_grad_(True)

    def step():
        Y = hgconv2(inc, X)
        (dX,) = torch.autograd.grad(Y, X, dY)
        return Y.detach(), dX.detach()

    Y0, dX0 = step()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    gc.collect()

    def caches():
        # everything the hops build lazily and keep: scales, folded weights, workspace sizes,
        # block-major copies
        out = [dict(inc._scales), dict(inc._edge_vals)]
        for o in (inc.csr, inc.csc):
            out += [dict(o._ws_bytes), dict(o._col_blocks), dict(o._blk_vals)]
        return out

    before = caches()
    graph_ = torch.cuda.CUDAGraph()
    # thread-local, as bench.py: autograd's device thread runs the backward during the capture
    with torch.cuda.graph(graph_, capture_error_mode="thread_local"):
        Yg, dXg = step()
    after = caches()
    assert len(before[0]) > 0 and len(before[1]) > 0  # the warm-up built them
    for b, a in zip(before, after):  # the captured step built nothing new: the same objects
        assert b.keys() == a.keys() and all(a[k] is b[k] for k in b)
    for _ in range(3):
        graph_.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(Yg, Y0) and torch.equal(dXg, dX0)
