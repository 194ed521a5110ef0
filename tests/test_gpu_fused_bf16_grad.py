"""``grad_dtype=torch.bfloat16`` of functional.two_hop_fused / att_two_hop_fused and of the KG
carriers' encoders: the fused row epilogue's backward stores dZ in bfloat16
(hgd_row_epilogue_backward_dt) and the first backward hop gathers that table. The cases, helpers
and bounds are tests/test_gpu_fused_bf16.py's.

Statements:
  * composition: with the option on, dX is bitwise the calls it is made of — the fp32 epilogue
    backward, ``.bfloat16()``, then the hops as spmm_csr calls — and Y, dγ, dβ and the residual
    gradients are bitwise those of the same call with ``gather_dtype`` alone;
  * off: ``grad_dtype=None`` is bitwise the call without the argument, with and without
    ``gather_dtype``; a pure blend (no LayerNorm, no activation: no kernel runs, dZ is dY) is
    bitwise the ``gather_dtype``-only call even with the option on;
  * against the float64 oracle on the bf16-rounded X: dX passes through one more bf16 store, the
    rounding of dZ, which adds at most 2^-9·|dZ| per element ahead of the linear chain, so it is
    held to tests/test_gpu_fused_bf16.py's bound with k + 1 stores,
    ((k+1)·2^-9·2 + 1e-5)·Σ|terms| (k = 1 for the two-hop, 3 for the attention form; the
    sign-of-z exemption is the one ``_check_rows`` applies at the rtol it is given). Y, dγ and dβ
    are not touched by the option and stay at their bounds with k.

``test_cpu_emulation_with_a_rounded_dz`` needs no device: the emulation of
tests/test_gpu_fused_bf16.py with dZ rounded by torch's CPU cast wherever the kernel would run,
against the same bounds. Its margins (largest error / bound over ``_all_cases()``): Y 0.250,
dX 0.901, dγ 0.012, dβ 0.000. The kernels' margins, printed by the GPU tests on an MI355X:
two_hop_fused Y 0.250, dX 0.901, dγ 0.010, dβ 0.001; att_two_hop_fused Y 0.196, dX 0.518,
dγ 0.012, dβ 0.002 — the emulation's.

Encoders: outputs bitwise those with ``gather_dtype`` alone (the forward is untouched). For the
gradients the reference is the fp32 path of the same encoder, and the bound is the Frobenius-norm
analogue of the ops' one, (K·2^-9·2 + 1e-5)·Σ|terms| with K the bf16 stores between the fp32
path and the result. An L-layer stack rounds, per layer, the table it gathers (bf16(x), or the
previous layer's bf16 copy) and its k intermediates on the way up, and dZ and its k intermediates
on the way down: K = 2·L·(k+1), to first order in 2^-9 (the forward's roundings reach a gradient
through act' and the LayerNorm statistics). Σ|terms| of a whole stack is not computed here;
‖g_fp32‖_F, which it is never below, stands in for it — the stricter choice:
    ‖g_on − g_fp32‖_F <= (2·L·(k+1)·2^-9·2 + 1e-5)·‖g_fp32‖_F     for x.grad and every dγ, dβ.
Measured on an MI355X, largest ‖g_on − g_fp32‖_F / ‖g_fp32‖_F over the gradients of an encoder
(bound), 2 / 3 layers: SelfAwareEncoder 5.9e-3 (3.1e-2) / 5.7e-3 (4.7e-2), RelationalAwareEncoder
6.6e-3 (3.1e-2) / 3.9e-3 (4.7e-2), KHGRecRelationalAwareEncoder 6.2e-3 (6.3e-2) / 8.3e-3 (9.4e-2).
The ``gather_dtype``-only path's deviation from the fp32 path is
printed next to it for comparison and asserted nowhere: a column sum such as a lower layer's dβ
moves up to 2.6 times as far with the option as without it (1.7e-3 of its norm against 0.7e-3,
SelfAwareEncoder, 2 layers) — presumably because the rounding of dZ is independent from row to
row while the roundings behind a hop are shared by the rows that gather them.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests.test_gpu_fused_bf16 import (ATT_WIDTHS, BF16, C_ATT, COMBOS, F32, M_ATT, N_ATT, NE,
                                       NV, UNALIGNED, WIDTHS, _all_cases, _att_case,
                                       _bf16_round, _check_rows, _emulate, _encoder_case,
                                       _epilogue_backward, _epilogue_desc, _fwd_bwd, _got, _inc,
                                       _kw, _norm, _rtol, _split_kw, _t, _two_hop_case)

gpu = pytest.mark.gpu

def _kernel_runs(o):
    return o["ln"] or o["act"] is not None


def _check_both(o, got, dX_k):
    """Y, dγ and dβ of ``got`` at the bound with k stores — ``_check_rows`` holds everything it
    is given to one rtol, so that pass takes ``dX_k``, a dX with k stores (the
    ``gather_dtype``-only one) — and the option's dX at the bound with k + 1. Returns the
    error / bound ratios of ``got``, each against its own bound."""
    k = o["k"]
    ratios = _check_rows(o, dict(got, dX=dX_k), _rtol(k))
    ratios["dX"] = _check_rows(o, got, _rtol(k + 1))["dX"]
    return ratios


# ---- the CPU emulation --------------------------------------------------------------------------
def _emulate16(o):
    """tests/test_gpu_fused_bf16.py's ``_emulate`` with the epilogue's dZ rounded to bf16 where
    the kernel runs (a pure blend hands dY on in fp32)."""
    ch, act, slope, ln = o["chain"], o["act"], o["slope"], o["ln"]
    gamma = beta = None
    if ln:
        gamma, beta = o["gamma"].astype(np.float64), o["beta"].astype(np.float64)
    res = o["res"]
    Z = ch.forward(o["Xr"], emulate=True)
    Y, _ = O.row_epilogue(Z, act, slope, ln, gamma, beta, 1e-5, o["out_scale"],
                          res[0] if res else None, o["s1"], res[1] if len(res) > 1 else None,
                          o["s2"])
    dZ, dg, db = O.row_epilogue_backward(Z, o["dY"], act, slope, ln, gamma, 1e-5, o["out_scale"])
    if _kernel_runs(o):
        dZ = _bf16_round(dZ)
    return dict(Y=Y, dX=ch.backward(dZ, emulate=True), dgamma=dg, dbeta=db)


def test_cpu_emulation_with_a_rounded_dz():
    """Every case through the emulation: dX against the bound with k + 1 stores, Y, dγ and dβ
    against theirs with k; prints the margins (largest error / bound)."""
    worst = {}
    for name, make in _all_cases():
        o = make()
        ratios = _check_both(o, _emulate16(o), _emulate(o)["dX"])
        print(f"emulation {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("emulation with a bf16 dZ, largest error / bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values())


# ---- the ops --------------------------------------------------------------------------------------
def _grads(f, o, dev, norm, dY, **kw):
    Xt = _t(o["X"], dev, True)
    rt = [_t(x, dev, True) for x in o["res"]]
    Y = f(Xt, **kw, **_kw(o, norm, rt))
    params = [Xt] + rt + ([norm.weight, norm.bias] if o["ln"] else [])
    grads = torch.autograd.grad(Y, params, dY)
    assert Y.dtype == F32 and all(g.dtype == F32 for g in grads)
    return Y.detach(), grads


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _run_op(o, dev, f, first_hops, last_hops, n_rows, csr, val, row_scale, name):
    """The three statements for one case. ``f(X, **kw)`` is the op; ``first_hops(X16)`` the
    forward's hops before the fused store over (``csr``, ``val``, ``row_scale``);
    ``last_hops(dZ, dz_scale)`` the backward's hops."""
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr_fused_dt
    norm = _norm(o, dev)
    dY = _t(o["dY"], dev)
    n_res = len(o["res"])
    Yg, gg = _grads(f, o, dev, norm, dY, gather_dtype=BF16)
    Y, g = _grads(f, o, dev, norm, dY, gather_dtype=BF16, grad_dtype=BF16)
    # the forward and everything but dX: the gather_dtype-only call's bits
    assert torch.equal(Y, Yg) and _same(g[1:], gg[1:])
    Y2, g2 = _grads(f, o, dev, norm, dY, gather_dtype=BF16, grad_dtype=BF16)
    assert torch.equal(Y, Y2) and _same(g, g2)
    # off: None is the call without the argument, with and without gather_dtype
    Yn, gn = _grads(f, o, dev, norm, dY, gather_dtype=BF16, grad_dtype=None)
    assert torch.equal(Yn, Yg) and _same(gn, gg)
    Y32, g32 = _grads(f, o, dev, norm, dY)
    Y32n, g32n = _grads(f, o, dev, norm, dY, grad_dtype=None)
    assert torch.equal(Y32, Y32n) and _same(g32, g32n)
    if not _kernel_runs(o):
        assert torch.equal(g[0], gg[0])  # the pure blend: no kernel, no cast pass
    else:
        assert not torch.equal(g[0], gg[0])  # it is another path
    # the calls dX is made of
    res = [_t(x, dev) for x in o["res"]]
    ex, epi, A, stats = _epilogue_desc(o, n_rows, dev, norm, res)
    Yc = spmm_csr_fused_dt(csr, first_hops(_t(o["X"], dev).bfloat16()), ex, val=val,
                           row_scale=row_scale)
    assert torch.equal(Yc, Y)
    dZ, dz_scale, dg, db = _epilogue_backward(o, epi, A, stats, norm, dY)
    if dz_scale == 1.0:
        dZ = dZ.bfloat16()
    dXc = last_hops(dZ, dz_scale)
    assert dXc.dtype == F32 and torch.equal(g[0], dXc)
    if o["ln"]:
        assert torch.equal(g[-2], dg) and torch.equal(g[-1], db)
    ratios = _check_both(o, _got(Y, g, n_res, o["ln"]), gg[0].cpu().numpy())
    print(f"{name} bf16 dZ d={o['d']}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def _run_two_hop(o, dev):
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    from hypergraph_diffusion_for_recommendation_amd.functional import two_hop_fused
    inc = _inc(o["r"], o["c"], o["vals"], (NV, NE), dev, **_split_kw(o["split"]))
    assert (inc.csr.n_heavy > 0) == o["split"]
    if "mask" in o:
        inc = inc.masked(torch.from_numpy(o["mask"]), 0.5)
    P, Q, R = o["P"], o["Q"], o["R"]
    q = inc.scale("col", Q)

    def f(X, **kw):
        return two_hop_fused(inc, X, P=P, Q=Q, R=R, **kw)

    def first_hops(X16):
        return spmm_csr(inc.csc, X16, val=inc.edge_values("csc", R), row_scale=q)

    def last_hops(dZ, dz_scale):
        qq = q
        if dz_scale != 1.0:
            qq = torch.full((NE,), dz_scale, device=dev) if q is None else q * dz_scale
        dM16 = spmm_csr(inc.csc, dZ, val=inc.edge_values("csc", P), row_scale=qq,
                        out_dtype=BF16)
        return spmm_csr(inc.csr, dM16, val=inc.val, row_scale=inc.scale("row", R),
                        out_dtype=F32)

    _run_op(o, dev, f, first_hops, last_hops, NV, inc.csr, inc.val, inc.scale("row", P),
            "two_hop_fused")


@gpu
@pytest.mark.parametrize("d", WIDTHS + UNALIGNED)
@pytest.mark.parametrize("ln", [False, True])
def test_two_hop_fused_bf16_grad(dev, d, ln):
    for i in range(len(COMBOS)):
        _run_two_hop(_two_hop_case(d, ln, i), dev)


@gpu
def test_two_hop_fused_bf16_grad_wide_row(dev):
    """d = 320 without LayerNorm: the epilogue's backward runs two column passes, the second
    over the last 64 columns."""
    _run_two_hop(_two_hop_case(320, False, 0), dev)


@gpu
def test_two_hop_fused_bf16_grad_masked_structure(dev):
    _run_two_hop(_two_hop_case(64, True, 0, masked=True), dev)


@gpu
def test_two_hop_fused_bf16_grad_empty_rows(dev):
    _run_two_hop(_two_hop_case(64, True, 3, empty_rows=True), dev)


@gpu
@pytest.mark.parametrize("d", ATT_WIDTHS)
@pytest.mark.parametrize("ln", [False, True])
def test_att_two_hop_fused_bf16_grad(dev, d, ln):
    from hypergraph_diffusion_for_recommendation_amd import spmm_csr
    from hypergraph_diffusion_for_recommendation_amd.functional import att_two_hop_fused
    for i in (0, 1):
        o = _att_case(d, ln, i)
        att = _inc(*o["att"], (N_ATT, M_ATT), dev, **_split_kw(o["split"]))
        inc = _inc(*o["kg"], (M_ATT, C_ATT), dev)

        def f(X, **kw):
            return att_two_hop_fused(att, inc, X, **kw)

        def hops(X, first):  # K·(Kᵀ·(attᵀ·X)), stored in bf16
            T = spmm_csr(att.csc, X, val=att.val_t, out_dtype=first)
            M = spmm_csr(inc.csc, T, val=inc.val_t)
            Z = spmm_csr(inc.csr, M, val=inc.val)
            assert T.dtype == M.dtype == Z.dtype == BF16
            return Z

        def last_hops(dZ, dz_scale):
            if dz_scale != 1.0:
                dZ = dZ * dz_scale
            return spmm_csr(att.csr, hops(dZ, BF16), val=att.val, out_dtype=F32)

        _run_op(o, dev, f, lambda X16: hops(X16, None), last_hops, N_ATT, att.csr, att.val, None,
                "att_two_hop_fused")


@gpu
@pytest.mark.parametrize("op", ["two_hop_fused", "att_two_hop_fused"])
def test_unfusable_shapes_keep_their_backward(dev, op):
    """LayerNorm at d = 320 and d = 100 and a negative slope take the unfused composition, whose
    backward has no fused epilogue kernel: bitwise the gather_dtype-only call with the option on."""
    from hypergraph_diffusion_for_recommendation_amd import functional as F
    for d, slope in ((320, 0.2), (100, 0.2), (64, -0.5)):
        o = (_two_hop_case if op == "two_hop_fused" else _att_case)(64, True, 0)
        rng = np.random.default_rng(d)
        norm = torch.nn.LayerNorm(d).to(dev)
        if op == "two_hop_fused":
            inc = _inc(o["r"], o["c"], o["vals"], (NV, NE), dev)
            n = NV

            def f(X, **kw):
                return F.two_hop_fused(inc, X, **kw)
        else:
            att = _inc(*o["att"], (N_ATT, M_ATT), dev)
            inc = _inc(*o["kg"], (M_ATT, C_ATT), dev)
            n = N_ATT

            def f(X, **kw):
                return F.att_two_hop_fused(att, inc, X, **kw)
        X = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
        res = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
        w = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
        outs = []
        for kw in (dict(), dict(grad_dtype=BF16)):
            Xg = X.clone().requires_grad_(True)
            Y = f(Xg, epilogue="leaky_relu", slope=slope, norm=norm, res1=res,
                  gather_dtype=BF16, **kw)
            grads = torch.autograd.grad(Y, [Xg, norm.weight, norm.bias], w)
            outs.append([Y.detach()] + list(grads))
        assert _same(outs[0], outs[1])


# ---- the encoders -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_layers", [2, 3])
@pytest.mark.parametrize("kind", ["self", "relational", "khgrec"])
def test_encoders_grad_dtype(dev, kind, n_layers):
    """Both attributes set: outputs bitwise the gather_dtype-only ones, every gradient within
    (2·L·(k+1)·2^-9·2 + 1e-5) of the fp32 path's in the Frobenius norm (module docstring, with
    the measured deviations)."""
    enc, call, chain, x, w = _encoder_case(kind, n_layers, dev)
    k = 3 if kind == "khgrec" else 1
    assert enc.grad_dtype is None
    fp32 = _fwd_bwd(enc, call, x, w)
    enc.gather_dtype = BF16
    gather = _fwd_bwd(enc, call, x, w)
    # a module without the attribute (one saved before it existed) is the gather_dtype-only one
    bare = copy.deepcopy(enc)
    del bare.grad_dtype
    assert not hasattr(bare, "grad_dtype")
    assert _same(_fwd_bwd(bare, call, x, w), gather)
    enc.grad_dtype = BF16
    on = _fwd_bwd(enc, call, x, w)
    assert _same(_fwd_bwd(enc, call, x, w), on)
    assert all(t.dtype == F32 for t in on) and len(on) == 2 + 2 * n_layers
    assert torch.equal(on[0], gather[0])  # the forward is untouched
    assert not torch.equal(on[1], gather[1])  # the backward is another path
    bound = _rtol(2 * n_layers * (k + 1))
    worst = 0.0
    for i, (a, g, r) in enumerate(zip(on[1:], gather[1:], fp32[1:])):
        scale = float(r.double().norm())
        assert scale > 0
        dev_on = float((a.double() - r.double()).norm()) / scale
        dev_gather = float((g.double() - r.double()).norm()) / scale
        print(f"{kind} L={n_layers} gradient {i}: ‖on − fp32‖ / ‖fp32‖ {dev_on:.2e}, "
              f"‖gather − fp32‖ / ‖fp32‖ {dev_gather:.2e}, bound {bound:.2e}")
        worst = max(worst, dev_on)
        assert dev_on <= bound, (kind, n_layers, i)
    print(f"{kind} L={n_layers}: largest deviation {worst:.2e} (bound {bound:.2e})")
    # off again: the fp32 path's bits
    enc.gather_dtype = enc.grad_dtype = None
    assert _same(_fwd_bwd(enc, call, x, w), fp32)
