"""GPU: KHGRec's KG attention (hgd_kg_attention_scores / _softmax, kg_attention.py), the
attention conv (layers.AttHGCNConv, functional.att_two_hop[_fused]) and KHGRec's KG encoder
against the float64 restatements of tests/_kg_ref64.py (the reference's own torch calls).

Bounds. Scores: the suite's 1e-5 of the sum of absolute terms. Softmax over given fp32 scores:
1e-5 of every probability (all terms positive), the other members of a duplicate run exactly 0.
End to end: the score bound propagated through the softmax — a probability's relative error is
at most 2·max δs over its row plus the softmax's own 1e-5, δs = 1e-5 · Σ mag over a run. The
convs: 1e-5 of |att|·|K|·|K|ᵀ·|att|ᵀ·|X|; behind a LayerNorm the row bound of the other LayerNorm
tests (tests/_ref64.check_rows)."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import _kg_ref64 as K
from tests import _ref64 as R64
from tests._util import RTOL, assert_close, random_coo

pytestmark = pytest.mark.gpu

N, NR = K.N_ENT, K.N_REL
# (d, dr): the KHGRec shape, narrow ones, widths that are no multiple of the 32-column pass or of
# the 16-byte row alignment, and one past every size limit of the score kernel (W_r larger than
# its LDS budget, more than one 128-column chunk of the rows, more than one 32-column pass)
WIDTHS = [(32, 32), (128, 32), (20, 32), (32, 24), (128, 24), (20, 24), (260, 40)]
ALL = tuple(range(NR))


@functools.lru_cache(maxsize=None)
def _triples(kind):
    if kind == "graph":
        return K.graph()
    return K.one_head(int(kind[len("one_head_"):]))


@functools.lru_cache(maxsize=None)
def _tables(d, dr):
    return K.tables(d, dr)


def _pattern(dev, trip, relations=None, **kw):
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import KGAttentionPattern
    h, t, r = (x.to(dev) for x in trip)
    return KGAttentionPattern(h, t, r, N, NR, relations, **kw)


# ---- 1. scores ------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dr,kind", [(d, dr, "graph") for d, dr in WIDTHS] + [
    (128, 32, "one_head_8192"), (20, 24, "one_head_8192")])  # many tiles of few relations
def test_scores(dev, d, dr, kind):
    trip = _triples(kind)
    E, W, R = _tables(d, dr)
    v = _pattern(dev, trip).scores(E.to(dev), W.to(dev), R.to(dev)).cpu()
    # the reference's loop concatenates relation by relation: `index` maps its order to the batch's
    _, _, ref, mag, index = K.scores(E, W, R, *trip, ALL)
    assert torch.equal(torch.sort(index).values, torch.arange(len(trip[0])))
    assert_close(v[index], ref, mag, what=f"scores d={d} dr={dr} {kind}")


def test_scores_many_relations(dev):
    """More relations than one 64-wide scan of the tile lookup holds, most of them empty, the
    used ones on both sides of the 64 and 128 boundaries."""
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import KGAttentionPattern
    n_rel, B, d, dr = 130, 400, 32, 24
    rng = np.random.default_rng(4)
    used = np.array([0, 5, 63, 64, 65, 127, 128, 129])
    h, t = (torch.from_numpy(rng.integers(0, N, B)) for _ in range(2))
    r = torch.from_numpy(used[rng.integers(0, len(used), B)])
    E, W, R = K.tables(d, dr, n_rel=n_rel)
    pat = KGAttentionPattern(h.to(dev), t.to(dev), r.to(dev), N, n_rel)
    v = pat.scores(E.to(dev), W.to(dev), R.to(dev)).cpu()
    _, _, ref, mag, index = K.scores(E, W, R, h, t, r, range(n_rel))
    assert_close(v[index], ref, mag, what="scores, 130 relations")
    # and with every second used relation disabled: the others' scores are unchanged
    keep = [int(q) for q in used[::2]]
    pat2 = KGAttentionPattern(h.to(dev), t.to(dev), r.to(dev), N, n_rel, keep)
    v2 = pat2.scores(E.to(dev), W.to(dev), R.to(dev)).cpu()
    on = torch.isin(r, torch.tensor(keep))
    assert torch.equal(v2[on], v[on])


def test_empty_batch(dev):
    """No triples: an attention without entries, and a conv that returns zeros."""
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import kg_attention
    from hypergraph_diffusion_for_recommendation_amd.layers import AttHGCNConv
    E, W, R = (x.to(dev) for x in _tables(32, 32))
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    att = kg_attention(E, e, e, e, W, R, N)
    assert att.nnz == 0 and int(att.csr.rowptr[-1]) == 0 and int(att.csc.rowptr[-1]) == 0
    _, _, inc, _ = _conv_case(dev, "identity", "plain")
    y = AttHGCNConv(0.2)(inc, att, E)
    assert y.shape == E.shape and not bool(y.any())


def test_scores_strided_tables(dev):
    """Rows of E and relation_emb that are views of wider tables (ldE > d, ldR > dr, rows not
    16-byte aligned)."""
    d, dr = 20, 24
    trip = _triples("graph")
    E, W, R = _tables(d, dr)
    Ew = torch.zeros(N, d + 3).to(dev)
    Rw = torch.zeros(NR, dr + 1).to(dev)
    Ew[:, :d] = E.to(dev)
    Rw[:, :dr] = R.to(dev)
    pat = _pattern(dev, trip)
    v = pat.scores(Ew[:, :d], W.to(dev), Rw[:, :dr])
    assert torch.equal(v, pat.scores(E.to(dev), W.to(dev), R.to(dev)))


# ---- 2. softmax alone -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,scale", [
    ("graph", 3.0), ("one_head_300", 2.0), ("one_head_8192", 0.3),
    # the row lengths at which the kernel changes hands: lane -> wave (8 / 9), wave -> workgroup
    ("one_head_8", 2.0), ("one_head_9", 2.0), ("one_head_512", 1.5), ("one_head_513", 1.5)])
def test_softmax(dev, kind, scale):
    """Chosen fp32 scores through hgd_kg_attention_softmax against torch.sparse.softmax in
    float64 over the same uncoalesced COO. The scales put the summed scores at O(1-10) (the long
    row's runs hold ~85 triples each)."""
    h, t, r = trip = _triples(kind)
    v = torch.randn(len(h), generator=torch.Generator().manual_seed(3)) * scale
    pat = _pattern(dev, trip)
    inc = pat.softmax(v.to(dev))
    ref = K.sparse_softmax_dense(h, t, v, N)
    first = pat.group_first().cpu()
    val = inc.val.cpu()
    assert bool((val[~first] == 0).all()), "a non-first member of a duplicate run is not 0"
    assert bool((val[first] > 0).all())
    assert int(first.sum()) == int((ref > 0).sum())
    got = K.dense_of(inc).double()
    err = ((got - ref).abs() / ref.clamp_min(1e-300))[ref > 0].max()
    print(f"softmax {kind}: max relative error {float(err):.3e}")
    assert_close(got, ref, ref, rtol=1e-5, what=f"softmax {kind}")  # (0 where the reference is)
    sums = got.sum(1)
    has = ref.sum(1) > 0
    assert bool((sums[~has] == 0).all())
    assert float((sums[has] - 1).abs().max()) <= 1e-5
    assert torch.equal(K.dense_of_t(inc), K.dense_of(inc))  # val_t: the same values, CSC order


# ---- 3. end to end --------------------------------------------------------------------------
@pytest.mark.parametrize("relations", [None, (0, 2, 3, 4), (0, 1, 2, 4)])
@pytest.mark.parametrize("d,dr", [(128, 32), (20, 24), (260, 40)])
def test_kg_attention_end_to_end(dev, d, dr, relations):
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import kg_attention
    h, t, r = trip = _triples("graph")
    E, W, R = _tables(d, dr)
    inc = kg_attention(E.to(dev), h.to(dev), t.to(dev), r.to(dev), W.to(dev), R.to(dev), N,
                       relations=None if relations is None else list(relations))
    ref, G = K.update_attention(E, W, R, h, t, r, ALL if relations is None else relations, N)
    got = K.dense_of(inc).double()
    ds = (RTOL * G).amax(1, keepdim=True)  # the row's largest score error
    assert_close(got, ref, ref * (2 * ds + 1e-5), rtol=1.0, what="attention")
    assert torch.equal(got > 0, ref > 0)  # a disabled relation's triples vanish
    assert torch.equal(K.dense_of_t(inc), K.dense_of(inc))
    rp = inc.csr.rowptr.cpu()
    live = sum(int((r == q).sum()) for q in (ALL if relations is None else relations))
    assert int(rp[-1]) == live
    if relations is not None and 3 not in relations:  # head 14's only triple is relation 3's
        assert int(rp[15] - rp[14]) == 0 and float(got[14].sum()) == 0.0
        assert int(inc.csc.rowptr[41] - inc.csc.rowptr[40]) == int(((t == 40) & (r != 3)).sum())


def test_kg_attention_all_on_one_head(dev):
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import kg_attention
    h, t, r = _triples("one_head_300")
    E, W, R = _tables(32, 32)
    inc = kg_attention(E.to(dev), h.to(dev), t.to(dev), r.to(dev), W.to(dev), R.to(dev), N)
    ref, G = K.update_attention(E, W, R, h, t, r, ALL, N)
    ds = (RTOL * G).amax(1, keepdim=True)
    assert_close(K.dense_of(inc).double(), ref, ref * (2 * ds + 1e-5), rtol=1.0)


# ---- 4. determinism -------------------------------------------------------------------------
def test_update_is_deterministic_and_order_free(dev):
    trip = _triples("graph")
    E, W, R = (x.to(dev) for x in _tables(128, 32))
    pat = _pattern(dev, trip)
    a, b = pat.update(E, W, R), pat.update(E, W, R)
    assert torch.equal(a.val, b.val) and torch.equal(a.val_t, b.val_t)
    # the same triples listed in another order: after coalescing, every value bit for bit (a
    # run's members stand in relation order and equal triples have equal scores, so only which
    # of several equal triples carries the value can change)
    p = torch.from_numpy(np.random.default_rng(9).permutation(len(trip[0])))
    c = _pattern(dev, tuple(x[p] for x in trip)).update(E, W, R)
    assert torch.equal(K.dense_of(c), K.dense_of(a))
    assert torch.equal(K.dense_of_t(c), K.dense_of(a))


# ---- 5. the conv ----------------------------------------------------------------------------
N_COLS = 60


@functools.lru_cache(maxsize=None)
def _adjacency():
    rng = np.random.default_rng(11)
    r, c = random_coo(rng, N, N_COLS, 500)
    vals = ((rng.random(len(r)) + 0.1) * 0.3).astype(np.float32)
    idx = torch.from_numpy(np.stack([r, c]))
    return idx, torch.from_numpy(vals)


def _conv_case(dev, att_kind, k_kind):
    """(att argument, att float64 dense, K argument, K float64 dense)."""
    from hypergraph_diffusion_for_recommendation_amd.incidence import Incidence
    idx, vals = _adjacency()
    inc = Incidence.from_coo(idx, vals, (N, N_COLS), device=dev)
    Kd = torch.zeros(N, N_COLS, dtype=torch.float64).index_put_((idx[0], idx[1]), vals.double())
    if k_kind == "dropped":
        keep = 0.7
        m = torch.from_numpy(np.random.default_rng(5).random(len(vals)) < keep)
        assert inc.coo_sorted  # the mask is in CSR order = the COO's order
        inc = inc.masked(m.to(dev), keep)
        Kd = torch.zeros_like(Kd).index_put_((idx[0][m], idx[1][m]),
                                             (vals[m] / np.float32(keep)).double())
    if att_kind == "identity":
        i = torch.arange(N)
        att = torch.sparse_coo_tensor(torch.stack([i, i]), torch.ones(N), (N, N)).to(dev)
        Ad = torch.eye(N, dtype=torch.float64)
    else:
        rel = None if att_kind == "update" else [0, 1, 2, 4]
        E, W, R = (x.to(dev) for x in _tables(32, 32))
        att = _pattern(dev, _triples("graph"), rel).update(E, W, R)
        Ad = K.dense_of(att).double()  # the fp32 attention is this test's input
        assert int((Ad.sum(1) == 0).sum()) >= 9 + (att_kind == "filtered")  # empty rows
    return att, Ad, inc, Kd


def _xw(d, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("k_kind", ["plain", "dropped"])
@pytest.mark.parametrize("att_kind", ["update", "filtered", "identity"])
def test_att_hgcn_conv(dev, att_kind, k_kind, act):
    from hypergraph_diffusion_for_recommendation_amd.layers import AttHGCNConv
    att, Ad, inc, Kd = _conv_case(dev, att_kind, k_kind)
    x, w = _xw(32)
    xg = x.to(dev).requires_grad_(True)
    y = AttHGCNConv(0.2)(inc, att, xg, act=act)
    (y * w.to(dev)).sum().backward()
    xc = x.double().requires_grad_(True)
    ref = K.att_conv(Ad, Kd, xc, act, 0.2)
    (ref * w.double()).sum().backward()
    M = Ad.abs() @ Kd.abs()
    M = M @ M.t()
    assert_close(y.detach().cpu(), ref.detach(), M @ x.double().abs(), what="Y")
    assert_close(xg.grad.cpu(), xc.grad, M @ w.double().abs(), what="dX")


@pytest.mark.parametrize("k_kind", ["plain", "dropped"])
def test_att_identity_is_hgcn_conv_bitwise(dev, k_kind):
    """With the reference's initial sparse_identity the attention hops gather one row with
    weight 1 (fmaf(1, x, 0) = x: they neither reorder nor round) and the activation runs in the
    last hop's store on the same pre-activation, so the result IS HGCNConv's, bit for bit."""
    from hypergraph_diffusion_for_recommendation_amd.layers import AttHGCNConv, HGCNConv
    att, _, inc, _ = _conv_case(dev, "identity", k_kind)
    x, w = _xw(32)
    outs = []
    for conv, args in ((AttHGCNConv(0.2), (inc, att)), (HGCNConv(0.2), (inc,))):
        for act in (True, False):
            xg = x.to(dev).requires_grad_(True)
            y = conv(*args, xg, act=act)
            (y * w.to(dev)).sum().backward()
            outs.append((y.detach(), xg.grad))
    for (ya, ga), (yb, gb) in zip(outs[:2], outs[2:]):
        assert torch.equal(ya, yb) and torch.equal(ga, gb)


def _affine_ln(d, dev, seed=0):
    from hypergraph_diffusion_for_recommendation_amd.layers import LayerNorm
    torch.manual_seed(seed)
    ln = LayerNorm(d).to(dev)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.2, 0.2)
    return ln


@pytest.mark.parametrize("slope,d", [(0.2, 32), (-0.1, 32), (0.2, 260)])
@pytest.mark.parametrize("k_kind", ["plain", "dropped"])
@pytest.mark.parametrize("att_kind", ["update", "filtered", "identity"])
def test_att_two_hop_fused(dev, att_kind, k_kind, slope, d):
    """LN(leaky(att·K·Kᵀ·attᵀ·X)) + res: forward, dX, dres, dγ, dβ. A negative slope and a
    LayerNorm over d > 256 are the shapes the fused store cannot hold (separate ops). A row of
    att without entries: β + res."""
    from hypergraph_diffusion_for_recommendation_amd.functional import att_two_hop_fused
    from hypergraph_diffusion_for_recommendation_amd.incidence import incidence_of
    att, Ad, inc, Kd = _conv_case(dev, att_kind, k_kind)
    att = incidence_of(att, cache=False)  # (the identity comes as a torch sparse tensor)
    x, w = _xw(d)
    res = torch.randn(N, d, generator=torch.Generator().manual_seed(7))
    ln = _affine_ln(d, dev)
    xg, rg = x.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    y = att_two_hop_fused(att, inc, xg, epilogue="leaky_relu", slope=slope, norm=ln, res1=rg)
    (y * w.to(dev)).sum().backward()
    lc = copy.deepcopy(ln).cpu().double()
    lc.weight.grad = lc.bias.grad = None
    xc, rc = x.double().requires_grad_(True), res.double().requires_grad_(True)
    z = K.att_conv(Ad, Kd, xc, True, slope)
    ref = torch.nn.functional.layer_norm(z, (d,), lc.weight, lc.bias, lc.eps) + rc
    (ref * w.double()).sum().backward()
    R64.check_rows(y, ref, "Y")
    R64.check_rows(xg.grad, xc.grad, "dX")
    R64.check_rows(rg.grad, rc.grad, "dres")
    R64.check_rows(ln.weight.grad, lc.weight.grad, "dgamma")
    R64.check_rows(ln.bias.grad, lc.bias.grad, "dbeta")
    empty = Ad.sum(1) == 0
    want = (ln.bias.detach().cpu() + res)[empty]
    torch.testing.assert_close(y.detach().cpu()[empty], want, rtol=1e-6, atol=0)


def test_att_identity_fused_is_two_hop_fused_bitwise(dev):
    """The fused form under the identity attention is two_hop_fused's, bit for bit."""
    from hypergraph_diffusion_for_recommendation_amd.functional import (att_two_hop_fused,
                                                                        two_hop_fused)
    from hypergraph_diffusion_for_recommendation_amd.incidence import incidence_of
    att, _, inc, _ = _conv_case(dev, "identity", "plain")
    att = incidence_of(att, cache=False)
    d = 32
    x, w = _xw(d)
    ln = _affine_ln(d, dev)
    outs = []
    for fn in (lambda xg: att_two_hop_fused(att, inc, xg, epilogue="leaky_relu", slope=0.2,
                                            norm=ln, res1=xg),
               lambda xg: two_hop_fused(inc, xg, epilogue="leaky_relu", slope=0.2, norm=ln,
                                        res1=xg)):
        xg = x.to(dev).requires_grad_(True)
        ln.weight.grad = ln.bias.grad = None
        y = fn(xg)
        (y * w.to(dev)).sum().backward()
        outs.append((y.detach(), xg.grad, ln.weight.grad.clone(), ln.bias.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_filtered_attention_under_forced_row_order(dev, monkeypatch):
    """HGD_SPMM_ROW_ORDER=1 forces the ordered walk wherever it applies — K's hops take it — but
    never on an attention pattern: with a `relations` filter its arrays run past rowptr[n]
    (the disabled triples), which a row order's gather permutation does not cover. Forward and
    backward of the conv and of the fused form, against float64."""
    from hypergraph_diffusion_for_recommendation_amd.functional import att_two_hop_fused
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_row_order
    from hypergraph_diffusion_for_recommendation_amd.layers import AttHGCNConv
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "1")
    att, Ad, inc, Kd = _conv_case(dev, "filtered", "plain")
    d = 32
    assert int(att.csr.rowptr[-1]) < att.nnz  # the capacity layout: a tail behind the last row
    assert spmm_row_order(inc.csr, d) and spmm_row_order(inc.csc, d)
    assert not spmm_row_order(att.csr, d) and not spmm_row_order(att.csc, d)
    x, w = _xw(d)
    M = Ad.abs() @ Kd.abs()
    M = M @ M.t()
    xg = x.to(dev).requires_grad_(True)
    y = AttHGCNConv(0.2)(inc, att, xg)
    (y * w.to(dev)).sum().backward()
    xc = x.double().requires_grad_(True)
    ref = K.att_conv(Ad, Kd, xc, True, 0.2)
    (ref * w.double()).sum().backward()
    assert_close(y.detach().cpu(), ref.detach(), M @ x.double().abs(), what="Y")
    assert_close(xg.grad.cpu(), xc.grad, M @ w.double().abs(), what="dX")
    assert att.csr._row_order is None and att.csc._row_order is None  # none was built
    ln = _affine_ln(d, dev)
    xg = x.to(dev).requires_grad_(True)
    y = att_two_hop_fused(att, inc, xg, epilogue="leaky_relu", slope=0.2, norm=ln, res1=xg)
    (y * w.to(dev)).sum().backward()
    lc = copy.deepcopy(ln).cpu().double()
    xc = x.double().requires_grad_(True)
    z = K.att_conv(Ad, Kd, xc, True, 0.2)
    ref = torch.nn.functional.layer_norm(z, (d,), lc.weight, lc.bias, lc.eps) + xc
    (ref * w.double()).sum().backward()
    R64.check_rows(y, ref, "Y fused")
    R64.check_rows(xg.grad, xc.grad, "dX fused")
    assert att.csr._row_order is None and att.csc._row_order is None


# ---- 6. the encoder -------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 128])
@pytest.mark.parametrize("n_layers", [2, 3])
def test_khgrec_relational_aware_encoder(dev, n_layers, d):
    from hypergraph_diffusion_for_recommendation_amd.encoders import KHGRecRelationalAwareEncoder
    _, _, inc, Kd = _conv_case(dev, "identity", "dropped")
    E, W, R = (x.to(dev) for x in _tables(d, 32))
    att = _pattern(dev, _triples("graph")).update(E, W, R)
    Ad = K.dense_of(att).double()
    torch.manual_seed(4)
    enc = KHGRecRelationalAwareEncoder(0.2, 0.1, n_layers, d).to(dev)
    assert sorted(enc.state_dict()) == sorted(
        f"lns.{i}.{p}" for i in range(n_layers) for p in ("weight", "bias"))
    assert [n for n, _ in enc.named_children()] == ["convs", "lns"]
    assert len(enc.convs) == n_layers
    with torch.no_grad():
        for ln in enc.lns:
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.uniform_(-0.2, 0.2)
    x, w = _xw(d)
    xg = x.to(dev).requires_grad_(True)
    out = enc(xg, inc, att)
    (out * w.to(dev)).sum().backward()
    ec = copy.deepcopy(enc).cpu().double()
    for p in ec.parameters():
        p.grad = None
    xc = x.double().requires_grad_(True)
    ref = K.relational_encoder(list(ec.lns), Ad, Kd, xc, 0.2)
    (ref * w.double()).sum().backward()
    R64.check_rows(out, ref, "out")
    R64.check_rows(xg.grad, xc.grad, "dX")
    for (n, p), (_, pc) in zip(enc.named_parameters(), ec.named_parameters()):
        R64.check_rows(p.grad, pc.grad, f"d {n}")


# ---- 7. no host synchronisation -------------------------------------------------------------
def test_no_host_synchronisation(dev):
    """A pattern built with validate=False, its update and the encoder's forward + backward run
    under torch's sync debug mode 'error', which raises on any synchronising call torch makes
    (.item(), .tolist(), a blocking copy). The library's own calls are stream-ordered launches."""
    from hypergraph_diffusion_for_recommendation_amd.encoders import KHGRecRelationalAwareEncoder
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import KGAttentionPattern
    d = 32
    _, _, inc, _ = _conv_case(dev, "identity", "dropped")
    E, W, R = (x.to(dev) for x in _tables(d, 32))
    h, t, r = (x.to(dev) for x in _triples("graph"))
    enc = KHGRecRelationalAwareEncoder(0.2, 0.1, 2, d).to(dev)
    x, w = (v.to(dev) for v in _xw(d))
    x.requires_grad_(True)
    want = KGAttentionPattern(h, t, r, N, NR, [0, 1, 2, 4]).update(E, W, R).val.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            h[:1].item()  # the mode does catch a host read on this build
        pat = KGAttentionPattern(h, t, r, N, NR, [0, 1, 2, 4], validate=False)
        att = pat.update(E, W, R)
        out = enc(x, inc, att)
        (out * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(att.val, want) and x.grad is not None
