"""Fused InfoNCE (csrc/infonce.hip) at every width, ragged split batches, the counted
(``batch_count``) path on poisoned scratch, the peaked regime of the diagonal split, the Python
group path and strided views — each against the reference's own formula in float64 on the host
(tests/_ref64.contrast_loss) on the same float32 inputs.

Bounds, all from the project: the loss within 1e-5 relative (test_gpu_infonce.py), every live
gradient row within ``_ref64.TOL`` of its largest |ref| (``_ref64.check_rows``), every table row
outside the batch exactly 0.0.

Input condition: a case is used only if the reference formula evaluated in float32 on the host
stays within TOL/4 of float64 by the same row measure (tests/test_infonce_geometry.py checks it
for the cases built here; part D is exempt — the float32 formula is useless there, which is the
point of that part).

The case builders (``case_*``) and the restatement of the slice planner (``slices_for``,
``per_slice``, ``plan``) are host-only; tests/test_infonce_geometry.py ties them to the library.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _ref64 as R

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# the slice planner of infonce.hip, restated (tests/test_infonce_geometry.py pins it to
# hgd_infonce_workspace_size)
# ---------------------------------------------------------------------------------------------
def slices_for(B: int) -> int:
    row_blocks = (B + 63) // 64
    s = (1024 + row_blocks - 1) // row_blocks
    return max(1, min(s, (B + 127) // 128))


def per_slice(B: int, S: int) -> int:
    return (-(-B // S) + 63) // 64 * 64


def plan(B: int):
    """(S, per_slice, S_used, rows of the last used slice) of a batch / capacity of B rows."""
    S = slices_for(B)
    ps = per_slice(B, S)
    used = -(-B // ps)
    return S, ps, used, B - (used - 1) * ps


def workspace_size(B: int, d: int) -> int:
    al = lambda n: -(-n // 256) * 256  # noqa: E731
    S = slices_for(B)
    return al(S * B * 4) + 2 * al(S * B * d * 4)


# ---------------------------------------------------------------------------------------------
# cases (host only)
# ---------------------------------------------------------------------------------------------
WIDTHS = list(range(16, 257, 16))
A_CASES = [(d, 0.2) for d in WIDTHS] + [(d, 0.05) for d in (80, 144, 240)]
B_SIZES = [15, 16, 17, 63, 64, 65, 128, 129, 145, 257, 513, 4999]
B_CASES = [(d, B) for d in (64, 80) for B in B_SIZES]
C_CAPACITY, C_N, C_TEMP = 300, 500, 0.2
C_COUNTS = [1, 2, 16, 17, 64, 65, 128, 129, 299, 300]
C_CASES = [(d, c) for d in (64, 96) for c in C_COUNTS]


def _tables(rng, N, d):
    return (rng.standard_normal((N, d)).astype(np.float32),
            rng.standard_normal((N, d)).astype(np.float32))


def case_width(d, temp):
    """Part A: N = 400, B = 193 unique nodes (two slices, the last of 65 rows: two full 32-row
    stages and a one-row stage)."""
    rng = np.random.default_rng(7000 + d + int(1000 * temp))
    E1, E2 = _tables(rng, 400, d)
    return E1, E2, rng.permutation(400)[:193].astype(np.int64), temp


@functools.lru_cache(maxsize=2)
def _geometry_tables(d):
    return _tables(np.random.default_rng(8000 + d), 6000, d)


def case_geometry(d, B):
    """Part B: N = 6000, τ = 0.2, B unique nodes."""
    E1, E2 = _geometry_tables(d)
    nodes = np.random.default_rng(8100 + d + B).permutation(6000)[:B].astype(np.int64)
    return E1, E2, nodes, 0.2


def case_counted(d, count):
    """Part C: a capacity-300 node list (three slices of 128) with ``count`` live ids — distinct
    table rows, a third of them written as negative ids, and from 16 live rows on one x / x − N
    pair on one table row (below that two equal batch rows are most of the batch and the true
    gradient cancels to nothing: the float32 formula fails the input condition there) — then
    garbage: 2^40, −2^40 and ids of rows that are not in the batch."""
    N, cap = C_N, C_CAPACITY
    rng = np.random.default_rng(9000 + 7 * d + count)
    E1, E2 = _tables(rng, N, d)
    perm = rng.permutation(N)
    rows = perm[:count].copy()
    if count >= 16:
        rows[1] = rows[0]
    ids = rows.astype(np.int64)
    neg = rng.random(count) < 1 / 3
    if count >= 16:
        neg[:2] = [False, True]  # the pair: x and x − N
    ids = np.where(neg, ids - N, ids)
    spare = perm[count:]  # rows outside the batch: a scatter to one of them shows
    tail = np.empty(cap - count, dtype=np.int64)
    tail[0::3] = 2 ** 40
    tail[1::3] = -2 ** 40
    tail[2::3] = spare[:len(tail[2::3])]
    return E1, E2, np.concatenate([ids, tail]), C_TEMP


def case_peaked(noise):
    """Part D: E2 = E1 + noise·randn at τ = 0.05, d = 64, N = 400, B = 193: p_bb ≈ 1."""
    rng = np.random.default_rng(11000 + int(100 * noise))
    E1 = rng.standard_normal((400, 64)).astype(np.float32)
    E2 = (E1 + np.float32(noise) * rng.standard_normal((400, 64)).astype(np.float32))
    return E1, E2.astype(np.float32), rng.permutation(400)[:193].astype(np.int64), 0.05


def case_single_row():
    """Part D: the B = 1 batch of test_infonce_single_row_batch."""
    E1, E2 = _tables(np.random.default_rng(11500), 100, 32)
    return E1, E2, np.array([7], dtype=np.int64), 0.3


E_U, E_N, E_D, E_TEMP, E_L = 700, 1900, 96, 0.3, 2


def case_layers():
    """Part E: two layers of [1900, 96] tables split at U = 700. The user list holds 130 distinct
    ids of [-40, 700) (capacity 130: S_used = 2, both slices live); the item list is 520 draws
    with replacement from [-60, 1200) (capacity 520: S_used = 5, about 420 live ids, so the last
    slice is empty)."""
    rng = np.random.default_rng(12000)
    tabs = [_tables(rng, E_N, E_D) for _ in range(E_L)]
    xu = (rng.permutation(740)[:130] - 40).astype(np.int64)
    xi = rng.integers(-60, E_N - E_U, size=520).astype(np.int64)
    return tabs, xu, xi


def reference(E1, E2, nodes, temp, dtype=torch.float64):
    """(loss, dE1, dE2) of the reference formula on the host in ``dtype``; negative ids index
    like torch."""
    c1 = torch.tensor(E1, dtype=dtype, requires_grad=True)
    c2 = torch.tensor(E2, dtype=dtype, requires_grad=True)
    loss = R.contrast_loss(c1, c2, torch.as_tensor(np.asarray(nodes)), temp)
    loss.backward()
    return float(loss.detach()), c1.grad, c2.grad


def row_ratio(got, ref) -> float:
    """The check_rows measure without the assertion (printed before asserting)."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = r.abs().amax(1)
    err = (g - r).abs().amax(1)
    return float((err / torch.where(scale == 0, torch.ones_like(scale), scale)).max())


def table_rows(nodes, N):
    rows = np.asarray(nodes, dtype=np.int64)
    return torch.from_numpy(np.unique(np.where(rows < 0, rows + N, rows)))


def check(tag, got, ref, rows, loss_check=True):
    """loss 1e-5 relative; rows ``rows`` of every given gradient by check_rows at TOL; every
    other row exactly zero; no NaN."""
    loss = got[0]
    grads = [(k, g.detach().double().cpu(), r)
             for k, (g, r) in enumerate(zip(got[1:], ref[1:]), 1) if g is not None]
    # every figure first, then the assertions
    if loss_check:
        rel = abs(loss - ref[0]) / abs(ref[0])
        print(f"{tag}: loss {loss:.9g} ref {ref[0]:.9g} rel {rel:.3e}")
    for k, g, r in grads:
        assert g.shape == r.shape
        print(f"{tag}: dE{k} worst row ratio {row_ratio(g[rows], r[rows]):.3e}")
    if loss_check:
        assert rel <= 1e-5, (tag, loss, ref[0])
    for k, g, r in grads:
        assert not bool(torch.isnan(g).any()), f"{tag}: NaN in dE{k}"
        R.check_rows(g[rows], r[rows], f"{tag} dE{k} rows")
        outside = torch.ones(g.shape[0], dtype=torch.bool)
        outside[rows] = False
        assert bool((g[outside] == 0).all()), f"{tag}: dE{k} nonzero outside the batch"


def run_public(dev, E1, E2, nodes, temp, count=None, need=(True, True)):
    from hypergraph_diffusion_for_recommendation_amd.functional import contrast_loss
    g1 = torch.from_numpy(E1).to(dev).requires_grad_(need[0])
    g2 = torch.from_numpy(E2).to(dev).requires_grad_(need[1])
    loss = contrast_loss(g1, g2, torch.from_numpy(nodes).to(dev), temp, count)
    loss.backward()
    return float(loss), g1.grad, g2.grad


# ---------------------------------------------------------------------------------------------
# A. every width, B. batch geometry
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,temp", A_CASES)
def test_every_width(dev, d, temp):
    """All sixteen instantiations of k_nce_rowsum / k_nce_bwd (and the masked lanes of the row
    kernels when group_for(d) > d/4) on a two-slice batch with a 65-row last slice."""
    E1, E2, nodes, temp = case_width(d, temp)
    check(f"A d={d} t={temp}", run_public(dev, E1, E2, nodes, temp),
          reference(E1, E2, nodes, temp), table_rows(nodes, 400))


@pytest.mark.parametrize("d,B", B_CASES)
def test_batch_geometry(dev, d, B):
    """Ragged batches around the 16-row wave, 32-row stage, 64-row block and slice edges
    (the geometry each B stands for is asserted in tests/test_infonce_geometry.py)."""
    E1, E2, nodes, temp = case_geometry(d, B)
    check(f"B d={d} B={B}", run_public(dev, E1, E2, nodes, temp),
          reference(E1, E2, nodes, temp), table_rows(nodes, 6000))


# ---------------------------------------------------------------------------------------------
# C. the counted path through the C ABI, every buffer owned (and poisoned) by the test
# ---------------------------------------------------------------------------------------------
class Counted:
    """One hgd_infonce term with a device count: scratch filled with NaN before the forward."""

    def __init__(self, dev, E1, E2, nodes, count, temp):
        from hypergraph_diffusion_for_recommendation_amd import _native as nat
        self.nat, self.lib, self.dev, self.temp = nat, nat.load(), dev, float(temp)
        self.E1, self.E2 = torch.from_numpy(E1).to(dev), torch.from_numpy(E2).to(dev)
        self.N, self.d = E1.shape
        self.nodes = torch.from_numpy(nodes).to(dev)
        self.cap = nodes.size
        self.count = torch.tensor([count], dtype=torch.int64, device=dev)
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
        self.P1, self.P2 = nan(self.cap, self.d), nan(self.cap, self.d)
        self.inv1, self.inv2, self.pos = nan(self.cap), nan(self.cap), nan(self.cap)
        self.deno = nan(2, self.cap)
        self.loss = nan(1)
        self.wsb = self.lib.hgd_infonce_workspace_size(self.cap, self.d)
        self.ws = nan(self.wsb // 4)
        self.grad = torch.ones(1, dtype=torch.float32, device=dev)

    def term(self, forward: bool):
        t = self.nat.InfonceTerm()
        if forward:
            t.E1, t.ld1, t.E2, t.ld2 = self.E1.data_ptr(), self.d, self.E2.data_ptr(), self.d
            t.pos_logit, t.loss = self.pos.data_ptr(), self.loss.data_ptr()
        t.n_rows, t.nodes, t.capacity = self.N, self.nodes.data_ptr(), self.cap
        t.batch_count = self.count.data_ptr()
        t.P1, t.P2 = self.P1.data_ptr(), self.P2.data_ptr()
        t.inv_norm1, t.inv_norm2 = self.inv1.data_ptr(), self.inv2.data_ptr()
        t.deno = self.deno.data_ptr()
        t.workspace, t.workspace_bytes = self.ws.data_ptr(), self.wsb
        return t

    def forward(self) -> float:
        nat, st = self.nat, self.nat.stream_handle(self.dev)
        nat.check(self.lib.hgd_infonce_forward_n(
            self.E1.data_ptr(), self.d, self.E2.data_ptr(), self.d, self.N,
            self.nodes.data_ptr(), self.cap, self.count.data_ptr(), self.d, self.temp,
            self.P1.data_ptr(), self.P2.data_ptr(), self.inv1.data_ptr(), self.inv2.data_ptr(),
            self.pos.data_ptr(), self.deno.data_ptr(), self.loss.data_ptr(), self.ws.data_ptr(),
            self.wsb, st), "hgd_infonce_forward_n")
        return float(self.loss)

    def backward(self, want1: bool, want2: bool):
        """hgd_infonce_backward_n into zeroed tables; the side not wanted is passed as NULL."""
        nat, st = self.nat, self.nat.stream_handle(self.dev)
        self.ws.fill_(float("nan"))
        z = lambda: torch.zeros((self.N, self.d), dtype=torch.float32, device=self.dev)  # noqa: E731
        dE1, dE2 = (z() if want1 else None), (z() if want2 else None)
        nat.check(self.lib.hgd_infonce_backward_n(
            self.P1.data_ptr(), self.P2.data_ptr(), self.inv1.data_ptr(), self.inv2.data_ptr(),
            self.deno.data_ptr(), self.cap, self.count.data_ptr(), self.d, self.temp,
            self.grad.data_ptr(), self.nodes.data_ptr(), self.N, nat.ptr(dE1), self.d,
            nat.ptr(dE2), self.d, self.ws.data_ptr(), self.wsb, st), "hgd_infonce_backward_n")
        return dE1, dE2


@pytest.mark.parametrize("d,count", C_CASES)
def test_counted_path_on_poisoned_scratch(dev, d, count):
    """hgd_infonce_forward_n / _backward_n at counts on the 16 / 32 / 64 / slice edges of a
    capacity of 300, with P1, P2, the norms, pos_logit, deno and the workspace full of NaN and
    garbage ids past the count: a read of a capacity row reaches the loss or a gradient as NaN,
    a scatter from one reaches a row outside the batch."""
    E1, E2, nodes, temp = case_counted(d, count)
    live = nodes[:count]
    rows = table_rows(live, C_N)
    ref = reference(E1, E2, live, temp)
    c = Counted(dev, E1, E2, nodes, count, temp)
    loss = c.forward()
    assert np.isfinite(loss)
    for want1, want2 in ((True, True), (True, False), (False, True)):
        dE1, dE2 = c.backward(want1, want2)
        tag = f"C d={d} count={count} sides={int(want1)}{int(want2)}"
        if count == 1:
            # the loss is log(1 + 1e-8·e^{-s/τ}) ≈ 0 (test_infonce_single_row_batch)
            assert abs(loss) < 1e-6
            for g in (dE1, dE2):
                if g is not None:
                    g = g.cpu()
                    assert bool(torch.isfinite(g).all())
                    outside = torch.ones(C_N, dtype=torch.bool)
                    outside[rows] = False
                    assert bool((g[outside] == 0).all())
            continue
        check(tag, (loss, dE1, dE2), ref, rows)


def test_counted_group_backward_into_compact_rows(dev):
    """hgd_infonce_backward_group with dX1 / dX2 and a count (a path Python never takes): the
    live rows are the reference's gradient rows of the gathered batch, the capacity rows —
    prefilled with NaN — exactly zero. A second term of the same launch wants dX1 alone (the
    dP2 side is then computed for it as well and dropped by the norm pass)."""
    d = 64
    cases = [case_counted(d, 129), case_counted(d, 17)]
    counts = [129, 17]
    cs = [Counted(dev, E1, E2, nodes, k, temp) for (E1, E2, nodes, temp), k in zip(cases, counts)]
    nat, lib = cs[0].nat, cs[0].lib
    terms = (nat.InfonceTerm * 2)()
    for i, c in enumerate(cs):
        terms[i] = c.term(forward=True)
    nat.check(lib.hgd_infonce_forward_group(terms, 2, d, C_TEMP, nat.stream_handle(dev)),
              "hgd_infonce_forward_group")
    outs = []
    for i, c in enumerate(cs):
        c.ws.fill_(float("nan"))
        t = c.term(forward=False)
        dX1 = torch.full((c.cap, d), float("nan"), dtype=torch.float32, device=dev)
        dX2 = torch.full((c.cap, d), float("nan"), dtype=torch.float32, device=dev)
        t.dX1 = dX1.data_ptr()
        if i == 0:
            t.dX2 = dX2.data_ptr()
        terms[i] = t
        outs.append((dX1, dX2 if i == 0 else None))
    nat.check(lib.hgd_infonce_backward_group(terms, 2, d, C_TEMP, cs[0].grad.data_ptr(),
                                             nat.stream_handle(dev)),
              "hgd_infonce_backward_group")
    for i, ((E1, E2, nodes, temp), k) in enumerate(zip(cases, counts)):
        live = nodes[:k]
        # the gathered rows as their own tables: row b of the gradient is batch row b's
        X1, X2 = E1[live], E2[live]
        ref = reference(X1, X2, np.arange(k), temp)
        loss = float(cs[i].loss)
        rel = abs(loss - ref[0]) / abs(ref[0])
        print(f"C group term {i}: loss rel {rel:.3e}")
        assert rel <= 1e-5
        for side, (g, r) in enumerate(zip(outs[i], ref[1:]), 1):
            if g is None:
                continue
            g = g.cpu()
            print(f"C group term {i}: dX{side} worst row ratio {row_ratio(g[:k], r):.3e}")
            R.check_rows(g[:k], r, f"group term {i} dX{side}")
            assert bool((g[k:] == 0).all()), f"group term {i}: dX{side} capacity rows not zero"


# ---------------------------------------------------------------------------------------------
# D. the peaked regime
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 0.1])
def test_peaked_regime_matches_float64(dev, noise):
    """E2 = E1 (+ 0.1·noise) at τ = 0.05: p_bb ≈ 1, the regime the diagonal split of infonce.hip
    exists for. The reference formula in float32 on the host is off by 0.28–0.33 of a gradient
    row's scale here and 1.6–2.5 % in the loss; the kernels are held to the float64 value at
    the bounds of every other case. Measured on an MI355X: gradient rows 6.5e-6 – 7.0e-6 of
    TOL's 1e-5 (a float64 recomputation from the kernels' stored float32 P1 / P2 is itself
    2.8e-6 – 4.5e-6 off: most of it is the rounding of the stored operands times 1/τ), loss
    1.4e-7. The loss was 4.9e-2 (noise 0) and 6.2e-3 (noise 0.1) off while k_nce_finish added
    the difference of the diagonal's two roundings, e_bb − nume_b, to the off-diagonal mass:
    this test found that."""
    E1, E2, nodes, temp = case_peaked(noise)
    check(f"D noise={noise}", run_public(dev, E1, E2, nodes, temp),
          reference(E1, E2, nodes, temp), table_rows(nodes, 400))


def test_single_row_batch_matches_float64(dev):
    """B = 1: loss = log1p(1e-8·e^{-s/τ}) ≈ 1e-8 and a gradient of that size, pure rounding noise
    in the float32 formula (row ratio 1.0); the kernels return the float64 value's digits."""
    E1, E2, nodes, temp = case_single_row()
    got = run_public(dev, E1, E2, nodes, temp)
    assert abs(got[0]) < 1e-6
    check("D B=1", got, reference(E1, E2, nodes, temp), table_rows(nodes, 100))


# ---------------------------------------------------------------------------------------------
# E. the Python group path
# ---------------------------------------------------------------------------------------------
def _layer_reference(tabs, un, pn, need):
    c = [[torch.tensor(t, dtype=torch.float64, requires_grad=n) for t, n in zip(pair, nd)]
         for pair, nd in zip(tabs, need)]
    un, pn = torch.as_tensor(un), torch.as_tensor(pn)
    total = 0
    for e1, e2 in c:
        total = total + R.contrast_loss(e1[:E_U], e2[:E_U], un, E_TEMP) \
            + R.contrast_loss(e1[E_U:], e2[E_U:], pn, E_TEMP)
    total.backward()
    return float(total), c


def test_layers_group_path_matches_float64(dev):
    """contrast_loss_layers (hgd_infonce_*_group on device counts) with mixed gradient needs —
    layer 0 wants E1 only, layer 1 both — against the float64 sum of its 2·L terms: the summed
    loss and every requested table gradient (the ``block[taken]`` bookkeeping and the in-kernel
    scatter into dE1), and no gradient for the table that asked for none."""
    from hypergraph_diffusion_for_recommendation_amd.functional import (contrast_loss_layers,
                                                                         unique_long_n)
    tabs, xu, xi = case_layers()
    need = [(True, False), (True, True)]
    un, uc = unique_long_n(torch.from_numpy(xu).to(dev), E_U)
    pn, pc = unique_long_n(torch.from_numpy(xi).to(dev), E_N - E_U)
    assert un.numel() == 130 and pn.numel() == 520
    ku, ki = int(uc), int(pc)
    assert ku == 130 and 384 < ki <= 512  # both user slices live; the fifth item slice empty
    g = [[torch.from_numpy(t).to(dev).requires_grad_(n) for t, n in zip(pair, nd)]
         for pair, nd in zip(tabs, need)]
    loss = contrast_loss_layers([p[0] for p in g], [p[1] for p in g], E_U, un, pn, E_TEMP, uc, pc)
    loss.backward()
    live_u, live_i = un[:ku].cpu().numpy(), pn[:ki].cpu().numpy()
    assert np.array_equal(live_u, np.unique(xu)) and np.array_equal(live_i, np.unique(xi))
    ref_loss, c = _layer_reference(tabs, live_u, live_i, need)
    rel = abs(float(loss) - ref_loss) / abs(ref_loss)
    print(f"E layers: loss rel {rel:.3e}")
    assert rel <= 1e-5
    rows = torch.cat([table_rows(live_u, E_U), E_U + table_rows(live_i, E_N - E_U)])
    for layer in range(E_L):
        for side in range(2):
            got, want = g[layer][side].grad, c[layer][side].grad
            if not need[layer][side]:
                assert got is None
                continue
            check(f"E layer {layer} side {side + 1}", (None, got), (None, want), rows,
                  loss_check=False)


def test_counted_call_with_detached_second_table(dev):
    """contrast_loss with a count, E1 requiring a gradient and E2 detached (the dE2 pointer is
    then NULL in hgd_infonce_backward_n)."""
    from hypergraph_diffusion_for_recommendation_amd.functional import (contrast_loss,
                                                                         unique_long_n)
    tabs, xu, _ = case_layers()
    E1, E2 = tabs[0][0][:E_U], tabs[0][1][:E_U]
    un, uc = unique_long_n(torch.from_numpy(xu).to(dev), E_U)
    g1 = torch.from_numpy(E1).to(dev).requires_grad_(True)
    g2 = torch.from_numpy(E2).to(dev)
    loss = contrast_loss(g1, g2, un, E_TEMP, uc)
    loss.backward()
    live = un[:int(uc)].cpu().numpy()
    assert g2.grad is None
    check("E counted E1-only", (float(loss), g1.grad), reference(E1, E2, live, E_TEMP)[:2],
          table_rows(live, E_U))


# ---------------------------------------------------------------------------------------------
# F. views
# ---------------------------------------------------------------------------------------------
def _view_case(dev, width, c0, counted):
    from hypergraph_diffusion_for_recommendation_amd.functional import (contrast_loss,
                                                                         unique_long_n)
    N, d, temp = 300, 64, 0.2
    rng = np.random.default_rng(13000 + width + c0)
    W1 = torch.from_numpy(rng.standard_normal((N, width)).astype(np.float32)).to(dev)
    W2 = torch.from_numpy(rng.standard_normal((N, width)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.permutation(N)[:150].astype(np.int64)).to(dev)
    nodes, count = unique_long_n(x, N) if counted else (x, None)
    outs = []
    for copy in (False, True):
        v1, v2 = W1[:, c0:c0 + d].detach(), W2[:, c0:c0 + d].detach()
        if copy:
            v1, v2 = v1.contiguous(), v2.contiguous()
        else:
            assert v1.stride() == (width, 1) and not v1.is_contiguous()
        v1.requires_grad_(True)
        v2.requires_grad_(True)
        loss = contrast_loss(v1, v2, nodes, temp, count)
        loss.backward()
        outs.append((loss.detach(), v1.grad, v2.grad))
    return outs


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("width,c0", [(192, 64), (128, 2), (66, 0)])
def test_column_slice_views_equal_their_copies(dev, width, c0, counted):
    """A column slice of a wider table — E[:, 64:128] of [N, 192] (aligned base, ld = 192 > d:
    read in place through ld1 / ld2), E[:, 2:66] of [N, 128] (base 8 bytes off a 16-byte
    boundary) and E[:, :64] of [N, 66] (rows not a multiple of four floats: both are copied,
    the kernels' float4 loads cannot read them) — gives bitwise the loss and both gradients of
    its contiguous copy. Unique nodes: no two batch rows meet in the scatter."""
    view, copy = _view_case(dev, width, c0, counted)
    for a, b in zip(view, copy):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(view[0])) and float(view[1].abs().max()) > 0
