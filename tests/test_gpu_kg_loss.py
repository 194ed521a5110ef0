"""GPU: KHGRec's TransR KG loss (hgd_kg_loss_forward / _backward, kg_loss.py) in its table form
(kg_loss) and its drop-in form (kg_loss_rows) against the float64 restatement of
tests/_kg_loss_ref64.py (the reference's own torch calls and autograd).

Bound: the suite's own, |got − ref64| <= 1e-5 · mag element-wise, for the loss, dE (or the three
row gradients), dW and dR; mag is the surrogate of _kg_loss_ref64 (absolute tables, differences
as sums, softplus as pos + neg) and its float64 autograd. An element whose mag is 0 — an empty
relation's dW and dR, an untouched row of dE — must be exactly 0. The reference's fp32 torch
calls stay within 2.3e-7 of mag at these shapes (on the CPU), so the bound has a factor 40 of
room for a different but fixed summation order."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import _kg_loss_ref64 as L
from tests import _kg_ref64 as K
from tests._util import RTOL, assert_close
from tests.test_gpu_kg_attention import WIDTHS as ATT_WIDTHS

pytestmark = pytest.mark.gpu

N, NR = K.N_ENT, K.N_REL
REG, BS = L.REG_KG, L.BATCH_SIZE_KG
# the attention tests' widths, the narrowest possible, and one whose W_r (32 KB) is over the
# score kernel's LDS budget; (260, 40) spans several column chunks and passes, (20, 24) has rows
# that are not 16-byte aligned; dr = 72 is more than one 64-column chunk of the backward's
# relation-space gradients, with W_r in LDS (20, 72) and read through the cache (140, 72)
WIDTHS = ATT_WIDTHS + [(4, 1), (128, 64), (20, 72), (140, 72)]


@functools.lru_cache(maxsize=None)
def _batch(kind):
    """(h, pos_t, neg_t, r) of a named batch."""
    if kind == "graph":
        h, t, r = K.graph()
    elif kind.startswith("one_head_"):
        h, t, r = K.one_head(int(kind[len("one_head_"):]))
    elif kind == "one":
        h, t, r = (x[:1].clone() for x in K.graph())
    elif kind == "one_relation_33":  # a full tile and a ragged second one
        rng = np.random.default_rng(6)
        h, t = (torch.from_numpy(rng.integers(0, N, 33)) for _ in range(2))
        r = torch.full((33,), 2, dtype=torch.int64)
    else:
        raise KeyError(kind)
    return h, t, L.neg_tails(t), r


@functools.lru_cache(maxsize=None)
def _tables(d, dr, scale=1.0, n_rel=NR):
    E, W, R = K.tables(d, dr, n_rel=n_rel)
    return E * scale, W, R * scale


@functools.lru_cache(maxsize=None)
def _reference(kind, d, dr, scale=1.0):
    h, t, n, r = _batch(kind)
    return L.reference(*_tables(d, dr, scale), h, t, n, r)


def _leaves(dev, tables, grads=(True, True, True)):
    return [x.to(dev).requires_grad_(g) for x, g in zip(tables, grads)]


def _run_table(dev, tables, batch, grads=(True, True, True), factor=None, **kw):
    """kg_loss forward + backward → (loss, dE, dW, dR) on the host (None where no gradient)."""
    from hypergraph_diffusion_for_recommendation_amd import kg_loss
    E, W, R = _leaves(dev, tables, grads)
    h, t, n, r = (x.to(dev) for x in batch)
    loss = kg_loss(E, h, t, n, r, W, R, REG, BS, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss if factor is None else factor(loss, E)).backward()
    return (loss.detach().cpu(), *(None if x.grad is None else x.grad.cpu() for x in (E, W, R)))


def _run_rows(dev, tables, batch):
    """kg_loss_rows over the gathered rows → (loss, [dX_h, dX_p, dX_n], dW, dR) on the host."""
    from hypergraph_diffusion_for_recommendation_amd import kg_loss_rows
    E, W, R = _leaves(dev, tables, (False, True, True))
    h, t, n, r = (x.to(dev) for x in batch)
    rows = [E[i].requires_grad_(True) for i in (h, t, n)]
    loss = kg_loss_rows(rows[0], r, rows[1], rows[2], W, R, REG, BS)
    loss.backward()
    return loss.detach().cpu(), [x.grad.cpu() for x in rows], W.grad.cpu(), R.grad.cpu()


def _check(got, ref, mag, what, rows=None):
    loss, dE, dW, dR = got
    print(f"{what}: loss {float(loss):.7g} ref {float(ref['loss']):.7g}")
    for name, g in (("loss", loss), ("dE", dE), ("dW", dW), ("dR", dR)):
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), f"{what}: {name} is not finite"
        err = float(((g.double() - ref[name]).abs() / mag[name].clamp_min(1e-300))
                    [mag[name] > 0].max()) if bool((mag[name] > 0).any()) else 0.0
        print(f"{what}: {name} max error {err:.3e} of mag")
        assert_close(g, ref[name], mag[name], what=f"{what} {name}")
    if rows is not None:
        for s, g in enumerate(rows):
            assert_close(g, ref["rows"][s], mag["rows"][s], what=f"{what} row gradient {s}")


# ---- 1. every width, both forms -------------------------------------------------------------
@pytest.mark.parametrize("d,dr", WIDTHS)
def test_widths_both_forms(dev, d, dr):
    tables, batch = _tables(d, dr), _batch("graph")
    ref, mag = _reference("graph", d, dr)
    got = _run_table(dev, tables, batch)
    _check(got, ref, mag, f"table d={d} dr={dr}")
    # the full-size outputs hold exact zeros where nothing contributes
    assert not bool(got[2][4].any()) and not bool(got[3][4].any())  # relation 4 is empty
    touched = torch.zeros(N, dtype=torch.bool).index_fill_(0, torch.cat(batch[:3]), True)
    assert not bool(got[1][~touched].any())
    loss_r, rows, dW_r, dR_r = _run_rows(dev, tables, batch)
    _check((loss_r, None, dW_r, dR_r), ref, mag, f"rows d={d} dr={dr}", rows=rows)
    assert torch.equal(loss_r, got[0])  # the forms differ in where the rows come from only
    assert torch.equal(dW_r, got[2]) and torch.equal(dR_r, got[3])
    # dE is the index_add of the row gradients (another, also fixed, order of the same terms)
    summed = torch.zeros(N, d, dtype=torch.float64)
    for idx, g in zip(batch[:3], rows):
        summed.index_add_(0, idx, g.double())
    assert_close(got[1], summed, mag["dE"], what="dE against the index_add of the row gradients")


# ---- 2. many tiles of three relations; one entity with 8192 positions in the scatter --------
@pytest.mark.parametrize("d,dr", [(128, 32), (20, 24)])
def test_one_head_8192(dev, d, dr):
    ref, mag = _reference("one_head_8192", d, dr)
    _check(_run_table(dev, _tables(d, dr), _batch("one_head_8192")), ref, mag,
           f"one head d={d} dr={dr}")


# ---- 3. more relations than one 64-wide scan holds ------------------------------------------
def test_many_relations(dev):
    """130 relations, most of them empty, the used ones on both sides of 64 and 128."""
    n_rel, B, d, dr = 130, 400, 32, 24
    rng = np.random.default_rng(4)
    used = np.array([0, 5, 63, 64, 65, 127, 128, 129])
    h, t = (torch.from_numpy(rng.integers(0, N, B)) for _ in range(2))
    r = torch.from_numpy(used[rng.integers(0, len(used), B)])
    batch = (h, t, L.neg_tails(t), r)
    tables = _tables(d, dr, 1.0, n_rel)
    ref, mag = L.reference(*tables, *batch)
    got = _run_table(dev, tables, batch)
    _check(got, ref, mag, "130 relations")
    empty = torch.ones(n_rel, dtype=torch.bool).index_fill_(0, torch.from_numpy(used), False)
    assert not bool(got[2][empty].any()) and not bool(got[3][empty].any())


# ---- 4, 5. the smallest batch; a ragged second tile -----------------------------------------
@pytest.mark.parametrize("kind", ["one", "one_relation_33"])
def test_small_batches(dev, kind):
    ref, mag = _reference(kind, 32, 32)
    _check(_run_table(dev, _tables(32, 32), _batch(kind)), ref, mag, kind)


# ---- 6. no triples --------------------------------------------------------------------------
def test_empty_batch_raises(dev):
    from hypergraph_diffusion_for_recommendation_amd import kg_loss, kg_loss_rows
    E, W, R = (x.to(dev) for x in _tables(32, 32))
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="empty batch"):
        kg_loss(E, e, e, e, e, W, R, REG, BS)
    with pytest.raises(ValueError, match="empty batch"):
        kg_loss_rows(E[:0], e, E[:0], E[:0], W, R, REG, BS)


# ---- 7. equal tails -------------------------------------------------------------------------
def test_negative_equals_positive(dev):
    """neg_t = pos_t throughout: both scores are bitwise equal, the loss is log 2 plus the
    regulariser."""
    d, dr = 32, 24
    h, t, _, r = _batch("graph")
    batch = (h, t, t.clone(), r)
    tables = _tables(d, dr)
    ref, mag = L.reference(*tables, *batch)
    E, W, R = (x.double() for x in tables)
    A, P = (torch.bmm(E[i].unsqueeze(1), W[r]).squeeze(1) for i in (h, t))
    want = math.log(2.0) + REG * (A.norm() + R[r].norm() + 2 * P.norm()) / BS
    got = _run_table(dev, tables, batch)
    assert_close(got[0], want, mag["loss"], what="log 2 + regulariser")
    _check(got, ref, mag, "neg = pos")


# ---- 8. tables of zeros ---------------------------------------------------------------------
def test_zero_tables(dev):
    """Every norm is exactly 0: it contributes 0 and a 0 gradient (as torch.norm does), the
    loss is softplus(0) = log 2 — the surrogate is 0 here, so the bound is 1e-5 of log 2."""
    tables = tuple(torch.zeros_like(x) for x in _tables(32, 24))
    loss, dE, dW, dR = _run_table(dev, tables, _batch("graph"))
    assert_close(loss, math.log(2.0), math.log(2.0), what="log 2")
    for name, g in (("dE", dE), ("dW", dW), ("dR", dR)):
        assert not bool(torch.isnan(g).any()), name
        assert not bool(g.any()), f"{name} is not exactly 0"


# ---- 9. saturated score differences ---------------------------------------------------------
def test_large_score_differences(dev):
    d, dr, scale = 32, 24, 40.0
    ref, mag = _reference("graph", d, dr, scale)
    assert float(ref["diff"].abs().max()) >= 1e4
    _check(_run_table(dev, _tables(d, dr, scale), _batch("graph")), ref, mag, "saturated")


# ---- 10. strided tables ---------------------------------------------------------------------
def test_strided_tables(dev):
    """ego_embed and relation_emb as views of wider tables (ldE > d, ldR > dr, rows not
    16-byte aligned): the same bits as from contiguous tables, and gradients of the views'
    shapes."""
    d, dr = 20, 24
    tables, batch = _tables(d, dr), _batch("graph")
    want = _run_table(dev, tables, batch)
    from hypergraph_diffusion_for_recommendation_amd import kg_loss
    Ew = torch.zeros(N, d + 3, device=dev)
    Rw = torch.zeros(NR, dr + 1, device=dev)
    Ew[:, :d] = tables[0].to(dev)
    Rw[:, :dr] = tables[2].to(dev)
    Ew.requires_grad_(True)
    Rw.requires_grad_(True)
    W = tables[1].to(dev).requires_grad_(True)
    h, t, n, r = (x.to(dev) for x in batch)
    loss = kg_loss(Ew[:, :d], h, t, n, r, W, Rw[:, :dr], REG, BS)
    loss.backward()
    assert torch.equal(loss.detach().cpu(), want[0])
    assert torch.equal(Ew.grad[:, :d].cpu(), want[1]) and not bool(Ew.grad[:, d:].any())
    assert torch.equal(W.grad.cpu(), want[2])
    assert torch.equal(Rw.grad[:, :dr].cpu(), want[3]) and not bool(Rw.grad[:, dr:].any())


# ---- 11. determinism ------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal(dev):
    tables, batch = _tables(128, 32), _batch("one_head_8192")
    a, b = _run_table(dev, tables, batch), _run_table(dev, tables, batch)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 12. a prebuilt pattern, its relations filter -------------------------------------------
def test_pattern_filter_does_not_affect_the_loss(dev):
    from hypergraph_diffusion_for_recommendation_amd import KGAttentionPattern
    tables, batch = _tables(128, 32), _batch("graph")
    h, t, _, r = (x.to(dev) for x in batch)
    pat = KGAttentionPattern(h, t, r, N, NR, relations=(0, 2))
    a = _run_table(dev, tables, batch, pattern=pat)
    b = _run_table(dev, tables, batch)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 13. index validation -------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_validate_raises_on_an_out_of_range_id(dev, which):
    from hypergraph_diffusion_for_recommendation_amd import kg_loss
    E, W, R = (x.to(dev) for x in _tables(32, 32))
    batch = [x.clone() for x in _batch("graph")]
    batch[which][17] = NR if which == 3 else N
    h, t, n, r = (x.to(dev) for x in batch)
    with pytest.raises(ValueError, match="out of range"):
        kg_loss(E, h, t, n, r, W, R, REG, BS)
    batch[which][17] = -1
    h, t, n, r = (x.to(dev) for x in batch)
    with pytest.raises(ValueError, match="out of range"):
        kg_loss(E, h, t, n, r, W, R, REG, BS, validate=True)


# ---- 14, 15. needs_input_grad ---------------------------------------------------------------
def test_only_trans_M_requires_grad(dev):
    tables, batch = _tables(128, 32), _batch("graph")
    full = _run_table(dev, tables, batch)
    loss, dE, dW, dR = _run_table(dev, tables, batch, grads=(False, True, False))
    assert dE is None and dR is None
    assert torch.equal(loss, full[0]) and torch.equal(dW, full[2])


def test_only_ego_embed_requires_grad(dev):
    tables, batch = _tables(128, 32), _batch("graph")
    full = _run_table(dev, tables, batch)
    loss, dE, dW, dR = _run_table(dev, tables, batch, grads=(True, False, False))
    assert dW is None and dR is None
    assert torch.equal(loss, full[0]) and torch.equal(dE, full[1])


# ---- 16. an incoming gradient other than 1 --------------------------------------------------
def test_scaled_loss_plus_another_term(dev):
    """(2.5 · loss + Σ E).backward(): dE = 2.5 · ref + 1 (mag 2.5 · mag + 1), dW and dR scale."""
    d, dr = 32, 24
    ref, mag = _reference("graph", d, dr)
    loss, dE, dW, dR = _run_table(dev, _tables(d, dr), _batch("graph"),
                                  factor=lambda loss, E: 2.5 * loss + E.sum())
    assert_close(loss, ref["loss"], mag["loss"], what="loss")
    assert_close(dE, 2.5 * ref["dE"] + 1, 2.5 * mag["dE"] + 1, what="dE")
    assert_close(dW, 2.5 * ref["dW"], 2.5 * mag["dW"], what="dW")
    assert_close(dR, 2.5 * ref["dR"], 2.5 * mag["dR"], what="dR")


# ---- 17. peak memory ------------------------------------------------------------------------
def test_peak_memory_is_below_the_reference_gather(dev):
    """Forward + backward at B = 4096, d = 64, dr = 32 stay below B·d·dr·4 bytes (33.5 MB) of
    extra device memory: the reference's trans_M[r] alone is that large. A condition, not a
    measurement: the arrays of this design ([3, B, dr], [3B, d], the tiles' partial dW, dW and
    the index work) total under 5 MB."""
    from hypergraph_diffusion_for_recommendation_amd import kg_loss
    B, d, dr = 4096, 64, 32
    _, t, r = K.one_head(B, seed=3)
    h = torch.from_numpy(np.random.default_rng(8).integers(0, N, B))
    E, W, R = _leaves(dev, K.tables(d, dr))
    h, t, n, r = (x.to(dev) for x in (h, t, L.neg_tails(t), r))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss = kg_loss(E, h, t, n, r, W, R, REG, BS)
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before
    print(f"peak extra device memory: {extra / 2 ** 20:.2f} MiB")
    assert extra < B * d * dr * 4
    assert bool(torch.isfinite(loss)) and E.grad is not None and W.grad is not None


# ---- 18. no host synchronisation ------------------------------------------------------------
def test_no_host_synchronisation(dev):
    """validate=False with a prebuilt pattern: forward and backward under torch's sync debug mode
    'error', which raises on any synchronising call torch makes."""
    from hypergraph_diffusion_for_recommendation_amd import KGAttentionPattern, kg_loss
    tables, batch = _tables(32, 32), _batch("graph")
    want = _run_table(dev, tables, batch)
    E, W, R = _leaves(dev, tables)
    h, t, n, r = (x.to(dev) for x in batch)
    pat = KGAttentionPattern(h, t, r, N, NR, validate=False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            h[:1].item()  # the mode does catch a host read on this build
        loss = kg_loss(E, h, t, n, r, W, R, REG, BS, pattern=pat, validate=False)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = (loss.detach().cpu(), E.grad.cpu(), W.grad.cpu(), R.grad.cpu())
    for x, y in zip(got, want):
        assert torch.equal(x, y)
