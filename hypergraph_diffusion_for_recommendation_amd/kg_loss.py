"""KHGRec's TransR knowledge-graph loss on the device (model/graph/KHGRec.py:347-365).

The reference's ``calculate_kg_loss`` runs on every minibatch (KHGRec.py:144) over the batch's
8192 sampled triples: ``W_r = self.trans_M[r]`` materialises a ``[B, d, dr]`` tensor (134 MB at
d = 128, dr = 32), three ``torch.bmm`` read it, and the backward writes a second one and folds it
back into ``trans_M`` with an ``index_put``. Here the batch is walked in its relation-grouped
order (the one :class:`~.kg_attention.KGAttentionPattern` already builds), a workgroup reads one
relation's ``W_r`` once per 32 triples, and the gradients of ``trans_M`` / ``relation_emb`` are
written whole from per-tile partial sums (``hgd_kg_loss_forward`` / ``hgd_kg_loss_backward``).

* :func:`kg_loss` is the table form: the rows are ``ego_embed[h]``, ``ego_embed[pos_t]``,
  ``ego_embed[neg_t]`` read through the indices (the gathers of KHGRec.py:124-126 are never
  materialised), and the gradient of ``ego_embed`` is one pull-style hop over the binary
  ``[n_entities, 3B]`` matrix "entity ← position" through the existing SpMM.
* :func:`kg_loss_rows` is the drop-in body of ``calculate_kg_loss`` over three gathered
  ``[B, d]`` tensors, with the reference's argument order.

Both are fp32, deterministic (every sum in a fixed order, no float atomics) and count a repeated
triple once per occurrence, as the reference's gathers do. Nothing is read back from the device
except the index check of ``validate=True``.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .incidence import CSR, DEFAULT_SPLIT_CHUNK, _stream, _ws, spmm_csr
from .kg_attention import KGAttentionPattern, _index_vector, _rowptr, _sort

__all__ = ["kg_loss", "kg_loss_rows"]


def _check_params(W, R, what: str):
    """dtype and shape checks of (trans_M, relation_emb); returns (n_relations, d, dr)."""
    for x, name in ((W, "trans_M"), (R, "relation_emb")):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be a float32 tensor, got "
                            f"{getattr(x, 'dtype', type(x).__name__)}")
    if W.dim() != 3 or R.dim() != 2:
        raise ValueError(f"{what}: expected trans_M [r, d, dr] and relation_emb [r, dr]; got "
                         f"{tuple(W.shape)}, {tuple(R.shape)}")
    n_rel, d, dr = (int(s) for s in W.shape)
    if R.shape[0] != n_rel:
        raise ValueError(f"{what}: trans_M / relation_emb hold {n_rel} / {R.shape[0]} relations")
    if R.shape[1] != dr:
        raise ValueError(f"{what}: relation_emb {tuple(R.shape)} does not match dr = {dr}")
    if d == 0 or dr == 0:
        raise ValueError(f"{what}: d and dr must be > 0")
    if n_rel == 0 or n_rel > 65535:
        raise ValueError(f"{what}: the relation count must be in [1, 65535], got {n_rel}")
    return n_rel, d, dr


def _check_scalars(reg_kg, batch_size_kg, what: str):
    reg_kg, bs = float(reg_kg), int(batch_size_kg)
    if bs <= 0:
        raise ValueError(f"{what}: batch_size_kg must be > 0, got {batch_size_kg}")
    return reg_kg, bs


def _check_devices(tensors, what: str) -> torch.device:
    dev = tensors[0][0].device
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: needs device (cuda/hip) tensors; there is no CPU path")
    for x, name in tensors[1:]:
        if x.device != dev:
            raise RuntimeError(f"{what}: {name} is on {x.device}, {tensors[0][1]} on {dev}")
    return dev


def _rows(x: torch.Tensor) -> torch.Tensor:
    """A strided view with unit column stride is read in place; anything else is copied."""
    x = x.detach()
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def _narrow(src: torch.Tensor, upper: int, flags: torch.Tensor, dev) -> torch.Tensor:
    """hgd_index_narrow: int64 ids → int32, an id outside [0, upper) counted in flags and
    replaced by 0."""
    src = src.to(dev).contiguous()
    dst = torch.empty(src.numel(), dtype=torch.int32, device=dev)
    nat.check(nat.load().hgd_index_narrow(src.data_ptr(), src.numel(), upper, dst.data_ptr(),
                                          flags.data_ptr(), _stream(dev)), "hgd_index_narrow")
    return dst


def scatter_csr(ids32, n_entities: int) -> CSR:
    """The binary ``[n_entities, P]`` matrix "entity ← position" of ``P`` int32 ids as a CSR:
    one stable sort, so a row lists its positions ascending. No values, no split plan and never
    the ordered walk, like the attention pattern's structures (it is rebuilt per batch)."""
    sorted_ids, perm = _sort(ids32, max(int(n_entities), 1))
    csr = CSR(_rowptr(sorted_ids, n_entities), perm, n_entities, ids32.numel(), 0,
              DEFAULT_SPLIT_CHUNK)
    csr.configure_kernel()
    csr.row_order_ok = False
    return csr


class _KGLoss(torch.autograd.Function):
    """hgd_kg_loss_forward / _backward. ``X1`` / ``X2`` None = the table form: all three row
    kinds are rows of ``X0`` through ``idx`` (int32 [3, B]); else ``idx`` is None."""

    @staticmethod
    def forward(ctx, X0, X1, X2, W, R, idx, grp_perm, rel_off, reg_kg, bs):
        lib = nat.load()
        dev = W.device
        n_rel, d, dr = W.shape
        table = X1 is None
        B = int(grp_perm.numel())
        xs = [_rows(X0)] * 3 if table else [_rows(X0), _rows(X1), _rows(X2)]
        Wc, Rc = W.detach().contiguous(), R.detach()
        if Rc.stride(1) != 1 or Rc.stride(0) < dr:
            Rc = Rc.contiguous()
        f = dict(dtype=torch.float32, device=dev)
        proj, coef = torch.empty((3, B, dr), **f), torch.empty(B, **f)
        norms, loss = torch.empty(4, **f), torch.empty((), **f)
        wsb = lib.hgd_kg_loss_workspace_size(B, n_rel, d, dr)
        ws = _ws(wsb, dev)
        src = []
        for s in range(3):
            src += [xs[s].data_ptr(), xs[s].stride(0), idx[s].data_ptr() if table else None]
        ctx.call = (*src, Wc.data_ptr(), Rc.data_ptr(), Rc.stride(0), n_rel, d, dr,
                    grp_perm.data_ptr(), rel_off.data_ptr(), B, reg_kg, bs)
        nat.check(lib.hgd_kg_loss_forward(*ctx.call, proj.data_ptr(), coef.data_ptr(),
                                          norms.data_ptr(), loss.data_ptr(), ws.data_ptr(), wsb,
                                          _stream(dev)), "hgd_kg_loss_forward")
        ctx.table, ctx.n_rows, ctx.wsb = table, int(X0.shape[0]), wsb
        # with what ctx.call points into, so that an in-place change before the backward is caught
        ctx.save_for_backward(proj, coef, norms, Wc, idx, *xs, Rc, grp_perm, rel_off)
        return loss

    @staticmethod
    def backward(ctx, g):
        proj, coef, norms, Wc, idx = ctx.saved_tensors[:5]
        lib = nat.load()
        dev = Wc.device
        n_rel, d, dr = Wc.shape
        B = coef.numel()
        need = ctx.needs_input_grad
        want_rows = need[0] if ctx.table else any(need[:3])
        want_params = need[3] or need[4]
        g = g.detach().to(dtype=torch.float32).reshape(1).contiguous()
        f = dict(dtype=torch.float32, device=dev)
        G = torch.empty((3 * B, d), **f) if want_rows else None
        dW = torch.empty((n_rel, d, dr), **f) if want_params else None
        dR = torch.empty((n_rel, dr), **f) if want_params else None
        if want_rows or want_params:
            ws = _ws(ctx.wsb, dev) if want_params else None
            nat.check(lib.hgd_kg_loss_backward(
                *ctx.call, proj.data_ptr(), coef.data_ptr(), norms.data_ptr(), g.data_ptr(),
                nat.ptr(G), nat.ptr(dW), nat.ptr(dR), nat.ptr(ws), ctx.wsb if want_params else 0,
                _stream(dev)), "hgd_kg_loss_backward")
        d0 = d1 = d2 = None
        if want_rows and ctx.table:
            # dE = S·G: entity ← its positions among the 3B rows of G, ascending
            d0 = spmm_csr(scatter_csr(idx.reshape(-1), ctx.n_rows), G)
        elif want_rows:
            d0, d1, d2 = (G[s * B:(s + 1) * B] if need[s] else None for s in range(3))
        return (d0, d1, d2, dW if need[3] else None, dR if need[4] else None, None, None, None,
                None, None)


def kg_loss(ego_embed: torch.Tensor, h: torch.Tensor, pos_t: torch.Tensor, neg_t: torch.Tensor,
            r: torch.Tensor, trans_M: torch.Tensor, relation_emb: torch.Tensor, reg_kg: float,
            batch_size_kg: int, pattern: KGAttentionPattern = None,
            validate: bool = True) -> torch.Tensor:
    """``calculate_kg_loss(ego_embed[h], r, ego_embed[pos_t], ego_embed[neg_t], reg_kg)``
    (KHGRec.py:124-126, :144, :347-365) as a 0-dim loss with autograd into ``ego_embed``,
    ``trans_M`` and ``relation_emb``; ``batch_size_kg`` is the configured ``self.batchSizeKG``
    the regulariser is divided by (the mean divides by the actual ``B``).

    ``pattern``: the batch's ``KGAttentionPattern(h, pos_t, r, …)`` if the caller has one; its
    narrowed ids and relation grouping are reused (its ``relations`` filter plays no part: the
    grouping covers all triples). Without one, the narrowing and the one sort by ``r`` are done
    here. ``validate``: read one error count back and raise ``ValueError`` on an index out of
    range; with ``validate=False`` nothing is read back and such an index is replaced by 0."""
    what = "kg_loss"
    n_rel, d, dr = _check_params(trans_M, relation_emb, what)
    if not isinstance(ego_embed, torch.Tensor) or ego_embed.dtype != torch.float32:
        raise TypeError(f"{what}: ego_embed must be a float32 tensor, got "
                        f"{getattr(ego_embed, 'dtype', type(ego_embed).__name__)}")
    if ego_embed.dim() != 2 or ego_embed.shape[1] != d:
        raise ValueError(f"{what}: ego_embed {tuple(ego_embed.shape)} does not match d = {d}")
    for x, name in ((h, "h"), (pos_t, "pos_t"), (neg_t, "neg_t"), (r, "r")):
        _index_vector(x, name, what)
    B = int(h.numel())
    if not (pos_t.numel() == neg_t.numel() == r.numel() == B):
        raise ValueError(f"{what}: h, pos_t, neg_t, r differ in length ({B}, {pos_t.numel()}, "
                         f"{neg_t.numel()}, {r.numel()})")
    if B == 0:
        raise ValueError(f"{what}: an empty batch has no loss (the reference returns NaN)")
    n_ent = int(ego_embed.shape[0])
    if n_ent == 0 or n_ent >= 2 ** 31 - 1 or 3 * B >= 2 ** 31 - 1:
        raise ValueError(f"{what}: sizes must be in [1, 2^31 - 1)")
    reg_kg, bs = _check_scalars(reg_kg, batch_size_kg, what)
    if pattern is not None and (pattern.B != B or pattern.n_entities != n_ent
                                or pattern.n_relations != n_rel
                                or pattern.h32.device != ego_embed.device):
        raise ValueError(f"{what}: the pattern is of {pattern.B} triples, {pattern.n_entities} "
                         f"entities, {pattern.n_relations} relations on {pattern.h32.device}; the "
                         f"call has {B}, {n_ent}, {n_rel} on {ego_embed.device}")
    dev = _check_devices([(ego_embed, "ego_embed"), (trans_M, "trans_M"),
                          (relation_emb, "relation_emb")], what)
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    n32 = _narrow(neg_t, n_ent, flags, dev)
    if pattern is not None:
        h32, t32, grp_perm, rel_off = pattern.h32, pattern.t32, pattern.grp_perm, pattern.rel_off
    else:
        h32, t32 = _narrow(h, n_ent, flags, dev), _narrow(pos_t, n_ent, flags, dev)
        r_sorted, grp_perm = _sort(_narrow(r, n_rel, flags, dev), n_rel)
        rel_off = _rowptr(r_sorted, n_rel)
    if validate and int(flags.item()):
        raise ValueError(f"{what}: {int(flags.item())} indices out of range for {n_ent} "
                         f"entities / {n_rel} relations")
    idx = torch.stack([h32, t32, n32])
    return _KGLoss.apply(ego_embed, None, None, trans_M, relation_emb, idx, grp_perm, rel_off,
                         reg_kg, bs)


def kg_loss_rows(h_embed: torch.Tensor, r: torch.Tensor, pos_t_embed: torch.Tensor,
                 neg_t_embed: torch.Tensor, trans_M: torch.Tensor, relation_emb: torch.Tensor,
                 reg_kg: float, batch_size_kg: int, validate: bool = True) -> torch.Tensor:
    """The body of ``calculate_kg_loss(h_embed, r, pos_t_embed, neg_t_embed, reg_kg)``
    (KHGRec.py:347-365) over three gathered ``[B, d]`` tensors, in the reference's argument order
    (``trans_M``, ``relation_emb`` and ``batch_size_kg`` are the model's attributes there).
    Gradients go to the three row tensors and to both parameters."""
    what = "kg_loss_rows"
    n_rel, d, dr = _check_params(trans_M, relation_emb, what)
    rows = ((h_embed, "h_embed"), (pos_t_embed, "pos_t_embed"), (neg_t_embed, "neg_t_embed"))
    for x, name in rows:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be a float32 tensor, got "
                            f"{getattr(x, 'dtype', type(x).__name__)}")
    _index_vector(r, "r", what)
    B = int(r.numel())
    for x, name in rows:
        if x.dim() != 2 or tuple(x.shape) != (B, d):
            raise ValueError(f"{what}: {name} {tuple(x.shape)} does not match {B} triples, "
                             f"d = {d}")
    if B == 0:
        raise ValueError(f"{what}: an empty batch has no loss (the reference returns NaN)")
    if 3 * B >= 2 ** 31 - 1:
        raise ValueError(f"{what}: sizes must be in [1, 2^31 - 1)")
    reg_kg, bs = _check_scalars(reg_kg, batch_size_kg, what)
    dev = _check_devices([*rows, (trans_M, "trans_M"), (relation_emb, "relation_emb")], what)
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    r_sorted, grp_perm = _sort(_narrow(r, n_rel, flags, dev), n_rel)
    rel_off = _rowptr(r_sorted, n_rel)
    if validate and int(flags.item()):
        raise ValueError(f"{what}: {int(flags.item())} relation ids out of range for {n_rel} "
                         f"relations")
    return _KGLoss.apply(h_embed, pos_t_embed, neg_t_embed, trans_M, relation_emb, None,
                         grp_perm, rel_off, reg_kg, bs)
