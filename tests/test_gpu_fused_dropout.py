"""GPU: the ED-HNN block's dropouts on the library RNG, in the Linear stores
(functional.dropout / linear_relu_dropout; layers2/EquivSetGNN2.py:91-101, HGNN_HD4.py:399).

* hgd_dropout_apply: the mask is oracle.dropout_keep_mask of the seed bit for bit, kept values
  × 1/(1-p); its backward is the same mask on the gradient;
* the row GEMM's dropout + residual epilogue gives bitwise relu(X·Wᵀ+b)·mask·scale + res on
  the same product, and its backward (mask from the stored activation, 1/(1-p) folded into W /
  dW / db) matches autograd of that composition;
* LocalAwareEncoder in train mode on the fused path (every dropout on the library RNG, the
  residual in the last Linear's store) against the float64 reference (tests/_ref64.py) fed the
  same masks, rebuilt from the recorded seeds: output rows, the ego gradient and every weight
  gradient at the 1e-5 bounds.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests import _ref64 as R

pytestmark = pytest.mark.gpu


def _mask(seed, shape, keep):
    return torch.from_numpy(O.dropout_keep_mask(seed, int(np.prod(shape)), keep).reshape(shape))


def test_dropout_kernel_is_the_oracle_mask(dev):
    from hypergraph_diffusion_for_recommendation_amd.functional import dropout
    g = torch.Generator(device=dev).manual_seed(0)
    for n, d, p in ((1000, 64, 0.5), (333, 12, 0.3), (7, 4, 0.9)):
        x = torch.randn(n, d, device=dev, generator=g).requires_grad_(True)
        seed = torch.tensor([123456789 + n], dtype=torch.int64, device=dev)
        y = dropout(x, p, seed)
        keep = 1.0 - p
        m = _mask(123456789 + n, (n, d), keep).to(dev)
        scale = float(torch.tensor(1.0 / keep, dtype=torch.float32))
        assert torch.equal(y, torch.where(m, x.detach() * scale, torch.zeros_like(y)))
        gy = torch.randn_like(y)
        (gx,) = torch.autograd.grad(y, x, gy)
        assert torch.equal(gx, torch.where(m, gy * scale, torch.zeros_like(gy)))
        frac = float(m.float().mean())
        assert abs(frac - keep) < 5 * (keep * (1 - keep) / m.numel()) ** 0.5 + 1e-3


@pytest.mark.parametrize("shape", [(5000, 32, 32), (777, 64, 128), (4096, 128, 64)])
def test_linear_relu_dropout_residual(dev, shape):
    from hypergraph_diffusion_for_recommendation_amd.functional import (linear,
                                                                         linear_relu_dropout)
    n, fi, fo = shape
    g = torch.Generator(device=dev).manual_seed(n)
    X = torch.randn(n, fi, device=dev, generator=g).requires_grad_(True)
    W = (0.2 * torch.randn(fo, fi, device=dev, generator=g)).requires_grad_(True)
    b = (0.1 * torch.randn(fo, device=dev, generator=g)).requires_grad_(True)
    res = torch.randn(n, fo, device=dev, generator=g).requires_grad_(True)
    p, keep = 0.5, 0.5
    seed = torch.tensor([987654 + n], dtype=torch.int64, device=dev)
    out = linear_relu_dropout(X, W, b, p, res=res, seed=seed)
    m = _mask(987654 + n, (n, fo), keep).to(dev)
    base = linear(X, W, b, relu=True)  # the same row-GEMM product, ReLU in its store
    ref = torch.where(m, base * 2.0, torch.zeros_like(base)) + res
    assert torch.equal(out, ref)
    G = torch.randn(n, fo, device=dev, generator=g)
    got = torch.autograd.grad(out, [X, W, b, res], G)
    exp = torch.autograd.grad(ref, [X, W, b, res], G)
    for name, a, e in zip(("X", "W", "b", "res"), got, exp):
        err = float((a - e).abs().max())
        assert err <= 1e-5 * float(e.abs().max()) + 1e-30, (name, err)


def test_local_aware_fused_dropout_train_matches_reference(dev, monkeypatch):
    """LocalAwareEncoder (HGNN_HD4.py:390-405), train mode, ED-HNN block dropout 0.5 on the
    fused path, last layer on the edge-dropped norm_adj (keep 0.8)."""
    from hypergraph_diffusion_for_recommendation_amd import layers
    from hypergraph_diffusion_for_recommendation_amd.encoders import LocalAwareEncoder
    from hypergraph_diffusion_for_recommendation_amd.layers import SpAdjDropEdge
    from tests.test_gpu_config_parity import (_check_params, _coo_host, _graph,
                                              _local_aware_reference)
    seeds = []

    def recorded_seed(device):
        s = 1000003 * (len(seeds) + 1)
        seeds.append(s)
        return torch.tensor([s], dtype=torch.int64, device=device)

    monkeypatch.setattr(layers, "dropout_seed", recorded_seed)
    U, I, nnz = 600, 900, 9000
    N, d, L = U + I, 32, 3
    ui, A = _graph(U, I, nnz, seed=40)
    data = SimpleNamespace(n_users=U, n_items=I, norm_adj=A, ui_adj=ui)
    torch.manual_seed(41)
    enc = LocalAwareEncoder(data, d, d, L, 0.3, 0.2, device=dev).train()
    assert all(blk._fused_dropout_ok() for blk in enc.edhnn_layers)
    g = torch.Generator().manual_seed(43)
    bound = (6.0 / (N + d)) ** 0.5
    ego = (torch.rand(N, d, generator=g) * 2 - 1) * bound
    G = torch.randn(N, d, generator=g)
    torch.manual_seed(44)
    dropped = SpAdjDropEdge()(enc.sparse_norm_adj, 0.8)
    x = ego.to(dev).requires_grad_(True)
    ue, ie = enc(x, dropped)
    out = torch.cat([ue, ie])
    out.backward(G.to(dev))
    assert len(seeds) == 3 * (L - 1)
    masks = [_mask(s, (N, d), 0.5) for s in seeds]

    idx, vals = _coo_host(enc.sparse_norm_adj)
    state = dict(enc.named_parameters())
    outR, gradsR, (di, dv), probe = _local_aware_reference(state, ui, idx, vals, U, I, d, L,
                                                           ego, G, masks, 0.5, 0.8, 44, None)
    gi, gv = _coo_host(dropped)
    assert torch.equal(di, gi) and torch.equal(dv, gv), "drop-edge structure"
    worst = R.check_rows(out, outR, "output")
    worst = max(worst, R.check_rows(x.grad, gradsR["ego"], "d ego"))
    worst = max(worst, _check_params({k: p.grad for k, p in state.items()}, gradsR, probe))
    print(f"LocalAware fused dropout: worst row ratio {worst:.2e}")


def test_module_path_unchanged_under_recorded_dropout(dev):
    """A block whose dropout is not exactly nn.Dropout (the tests' recorded-mask dropout) takes
    the module path; eval mode takes the fused path without dropout: both give the eval output
    of the module path."""
    from hypergraph_diffusion_for_recommendation_amd.encoders import LocalAwareEncoder
    U, I, nnz = 300, 400, 4000
    ui, A = None, None
    from tests.test_gpu_config_parity import _graph
    ui, A = _graph(U, I, nnz, seed=50)
    data = SimpleNamespace(n_users=U, n_items=I, norm_adj=A, ui_adj=ui)
    torch.manual_seed(51)
    enc = LocalAwareEncoder(data, 32, 32, 3, 0.3, 0.2, device=dev).eval()
    x = torch.randn(U + I, 32, device=dev)
    with torch.no_grad():
        a = torch.cat(enc(x, enc.sparse_norm_adj))
        for blk in enc.edhnn_layers:
            blk.fused_dropout = False
        b = torch.cat(enc(x, enc.sparse_norm_adj))
    err = float((a - b).abs().max())
    assert err <= 1e-6 * float(b.abs().max()), err


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_dense_hypergraph_block_respects_aggr(dev, aggr):
    """A block on a DENSE hypergraph (HCCF_diffusion.py:205-206) takes the dense mean fast path
    only for aggr='mean'; with 'add' (EquivSetConv's default) it must sum, as the module path
    over V/E = nonzero(H > 0) does. Eval mode: both paths deterministic."""
    from hypergraph_diffusion_for_recommendation_amd.layers import EquivSetGNN
    from hypergraph_diffusion_for_recommendation_amd.encoders import edhnn_config
    n, K, d = 700, 32, 32
    args = dict(edhnn_config(d), aggregate=aggr)
    torch.manual_seed(52)
    blk = EquivSetGNN(d, args).to(dev).eval()
    g = torch.Generator().manual_seed(53)
    H = torch.randn(n, K, generator=g).to(dev)
    x = torch.randn(n, d, generator=g).to(dev)
    Hu, Hi = H[:300].contiguous(), H[300:].contiguous()
    with torch.no_grad():
        fast = blk(x, H, n)
        pair_ok = blk.dense_pair_ok(x, Hu, Hi)
        blk.fused_dropout = False
        ref = blk(x, H, n)
    assert pair_ok == (aggr == "mean")
    err = float((fast - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), (aggr, err)


def _mean_pair64(H, X, G):
    """Float64 restatement of the scatter-mean pair over nonzero(H > 0) and its backward."""
    B = (H > 0).double().cpu()
    ce = B.sum(0).clamp_min(1.0)
    cv = B.sum(1).clamp_min(1.0)
    Xe = (B.t() @ X.detach().double().cpu()) / ce[:, None]
    Y = (B @ Xe) / cv[:, None]
    dX = B @ ((B.t() @ (G.double().cpu() / cv[:, None])) / ce[:, None])
    return Y, dX


@pytest.mark.parametrize("n,K,d", [(3000, 32, 64), (517, 16, 32), (2048, 128, 128),
                                   (517, 32, 272)])
def test_dense_mean_two_hop_matches_the_vertex_edge_means(dev, n, K, d):
    """functional.dense_mean_two_hop (V/E = nonzero(H > 0) of a dense learned hypergraph,
    HCCF_diffusion.py:382-402 + the torch_scatter mean pair) against the float64 restatement of
    the two scatter means, forward and backward; rows and columns without a positive entry
    included (their means are 0). d = 272 is the Python route to N > 128 on hgd_gemm_rows
    (three column slices of the staged kernel, the last one ragged)."""
    from hypergraph_diffusion_for_recommendation_amd.functional import dense_mean_two_hop
    g = torch.Generator(device=dev).manual_seed(n + K)
    H = torch.randn(n, K, device=dev, generator=g)
    H[:7] = -1.0          # vertices without hyperedges
    H[:, 3] = -1.0        # a hyperedge without vertices
    X = torch.randn(n, d, device=dev, generator=g).requires_grad_(True)
    Y = dense_mean_two_hop(H, X)
    G = torch.randn(n, d, device=dev, generator=g)
    (dX,) = torch.autograd.grad(Y, X, G)
    Yr, dXr = _mean_pair64(H, X, G)
    R.check_rows(Y, Yr, "Y")
    R.check_rows(dX, dXr, "dX")
    assert not Y[:7].any()


@pytest.mark.parametrize("nu,ni,K,d", [(3000, 2500, 32, 64), (17, 700, 16, 32), (1024, 64, 128, 16)])
def test_dense_mean_two_hop_pair_is_the_two_halves(dev, nu, ni, K, d):
    """dense_mean_two_hop_pair (HCCF_diffusion's user and item calls of the block as one grouped
    op over one [N, d] table) against the float64 restatement of each half, forward and
    backward."""
    from hypergraph_diffusion_for_recommendation_amd.functional import dense_mean_two_hop_pair
    g = torch.Generator(device=dev).manual_seed(nu + ni)
    Hu = torch.randn(nu, K, device=dev, generator=g)
    Hi = torch.randn(ni, K, device=dev, generator=g)
    Hu[:3] = -1.0
    Hi[:, 1] = -1.0
    X = torch.randn(nu + ni, d, device=dev, generator=g).requires_grad_(True)
    Y = dense_mean_two_hop_pair(Hu, Hi, X)
    G = torch.randn(nu + ni, d, device=dev, generator=g)
    (dX,) = torch.autograd.grad(Y, X, G)
    Yu, dXu = _mean_pair64(Hu, X[:nu], G[:nu])
    Yi, dXi = _mean_pair64(Hi, X[nu:], G[nu:])
    R.check_rows(Y, torch.cat([Yu, Yi]), "Y")
    R.check_rows(dX, torch.cat([dXu, dXi]), "dX")


@pytest.mark.parametrize("pair", [True, False])
def test_hccf_diffusion_dense_fused_train_matches_reference(dev, monkeypatch, pair):
    """HCCFDiffusionEncoder (HCCF_diffusion.py:131-215), train mode, on the fused path: the ED-HNN
    block on the dense learned hypergraph through dense_mean_two_hop, its dropouts on the
    library RNG (masks rebuilt from the recorded seeds), against the float64 reference."""
    from hypergraph_diffusion_for_recommendation_amd import layers
    from hypergraph_diffusion_for_recommendation_amd.encoders import HCCFDiffusionEncoder
    from tests.test_gpu_config_parity import _check_params, _coo_host, _graph
    seeds = []

    def recorded_seed(device):
        s = 7919 * (len(seeds) + 3) + (len(seeds) << 33)
        seeds.append(s)
        return torch.tensor([s], dtype=torch.int64, device=device)

    monkeypatch.setattr(layers, "dropout_seed", recorded_seed)
    U, I, nnz, d, L = 1_200, 1_500, 20_000, 32, 2
    N = U + I
    _, A = _graph(U, I, nnz, seed=60)
    data = SimpleNamespace(n_users=U, n_items=I, norm_adj=A)
    kw = dict(lrate=1e-3, lr_decay=0.9, max_epoch=1, batch_size=64, reg=0.01,
              embedding_size=d, hyper_dim=32, drop_rate=0.2, p=0.3, n_layers=L)
    torch.manual_seed(61)
    enc = HCCFDiffusionEncoder(kw, data, device=dev).train()
    assert enc.edhnnlayer._fused_dropout_ok()
    if not pair:  # the per-call path (one block call per row block, three seeds each)
        monkeypatch.setattr(enc.edhnnlayer, "dense_pair_ok", lambda *a: False)
    enc.drop_out = R.FixedDropout(0.2, 62)
    enc.edgeDropper = R.DropRecorder(enc.edgeDropper)
    torch.manual_seed(64)
    ue, ie, gcns, hyps = enc(keep_rate=0.7)
    g = torch.Generator().manual_seed(65)
    Gu, Gi = torch.randn(U, d, generator=g), torch.randn(I, d, generator=g)
    Gh = [torch.randn(N, d, generator=g) for _ in range(L)]
    tot = (ue * Gu.to(dev)).sum() + (ie * Gi.to(dev)).sum()
    for layer in range(L):
        tot = tot + (hyps[layer] * Gh[layer].to(dev)).sum()
    tot.backward()
    blk_masks = []
    if pair:  # three [N, d] masks per layer: their user rows, then their item rows
        assert len(seeds) == 3 * L
        for layer in range(L):
            ms = [_mask(s, (N, d), 0.5) for s in seeds[3 * layer:3 * layer + 3]]
            blk_masks += [m[:U] for m in ms] + [m[U:] for m in ms]
    else:
        assert len(seeds) == 3 * 2 * L
        for k, s in enumerate(seeds):
            rows = U if (k // 3) % 2 == 0 else I
            blk_masks.append(_mask(s, (rows, d), 0.5))

    P = R.leaves(enc)
    idx, vals = _coo_host(enc.sparse_norm_adj)
    torch.manual_seed(64)
    adjs = []
    for layer in range(L):
        di, dv = R.drop_edge_reference(idx, vals, 0.7)
        gi, gv = enc.edgeDropper.outputs[layer]
        assert torch.equal(di, gi) and torch.equal(dv, gv), f"drop-edge layer {layer}"
        adjs.append(R.sparse(di, dv, (N, N)))
    probe = R.Probe()
    ueR, ieR, gR, hR = R.hccf_diffusion(P, adjs, enc.drop_out.masks, 0.8, blk_masks, 0.5, U, L,
                                        1e-5, None, probe)
    worst = max(R.check_rows(ue, ueR, "user_emb"), R.check_rows(ie, ieR, "item_emb"))
    for layer in range(L):
        worst = max(worst, R.check_rows(gcns[layer], gR[layer], f"gcn[{layer}]"),
                    R.check_rows(hyps[layer], hR[layer], f"hyper[{layer}]"))
    totR = (ueR * Gu.double()).sum() + (ieR * Gi.double()).sum()
    for layer in range(L):
        totR = totR + (hR[layer] * Gh[layer].double()).sum()
    totR.backward()
    got = {k: p.grad for k, p in enc.named_parameters()}
    gradsR = {k: v.grad for k, v in P.items()}
    for k in ("embedding_dict.user_w", "embedding_dict.item_w"):  # structure only: no gradient
        assert gradsR[k] is None and (got[k] is None or not got[k].any()), k
        got[k] = gradsR[k] = None
    worst = max(worst, _check_params(got, gradsR, probe))
    print(f"HCCF_diffusion dense fused (pair={pair}): worst row ratio {worst:.2e}")
