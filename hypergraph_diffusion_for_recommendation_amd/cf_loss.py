"""KHGRec's CF loss on the device over the batch's item rows only (model/graph/KHGRec.py:131-143
and ``calculate_cf_loss``, :341-345).

The reference fuses the two views of EVERY item on every minibatch and then reads the 2·B rows
the batch names::

    item_emb_fused, _ = self.attention_item(torch.stack([item_emb_cf, item_emb_kg], dim=1))
    anchor, pos, neg = user_emb_cf[uid], item_emb_fused[pid], item_emb_fused[nid]
    cf_loss = bpr_loss(anchor, pos, neg) + l2_reg_loss(reg, anchor, pos, neg) / batchSize

Every other row's gradient is exactly zero and the fusion's backward is linear in dOut, so the
fusion evaluated at the batch's positions is the same function with the same gradients.
:func:`cf_loss` does that: one row kernel reads both views through the ids, fuses, scores and
sums (the fused rows never reach memory), one backward kernel returns the per-position gradients
(``hgd_cf_loss_forward`` / ``hgd_cf_loss_backward``), and the three table gradients are pull-style
hops over :func:`~.kg_loss.scatter_csr`, as for the KG loss. Work and extra memory are O(B·d).

fp32, deterministic (every sum in a fixed order, no float atomics); a repeated id counts once per
occurrence. Nothing is read back from the device except the index check of ``validate=True``.
:func:`cf_loss_supported` says which path a call takes: widths outside the fused set, misaligned
rows and CPU tensors run the reference's expression in torch.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _native as nat
from .incidence import _stream, _ws, spmm_csr
from .kg_attention import _index_vector
from .kg_loss import _narrow, scatter_csr

__all__ = ["cf_loss", "cf_loss_supported"]


def _rows_ok(x: torch.Tensor, d: int) -> bool:
    """A [n, d] view the kernels read in place: unit column stride, 16-byte aligned rows."""
    return (x.stride(1) == 1 and (x.shape[0] <= 1 or (x.stride(0) >= d and x.stride(0) % 4 == 0))
            and x.data_ptr() % 16 == 0)


def _ld(x: torch.Tensor, d: int) -> int:
    return x.stride(0) if x.shape[0] > 1 else d


def _rows(x: torch.Tensor) -> torch.Tensor:
    """Unit column stride is read in place; anything else is copied."""
    x = x.detach()
    return x if x.stride(1) == 1 else x.contiguous()


def _width_ok(d: int, attention: bool) -> bool:
    return (d % 16 == 0 and 16 <= d <= 128) if attention else (d % 4 == 0 and 4 <= d <= 256)


def cf_loss_supported(user_emb: torch.Tensor, item_cf: torch.Tensor, item_kg: torch.Tensor,
                      W1=None, b1=None, W2=None) -> bool:
    """True when a call with these tensors runs the fused kernels: device float32 tensors, a
    width in the mode's set (attention: a multiple of 16 in [16, 128]; mean: a multiple of 4 up
    to 256) and rows that are 16-byte aligned (pointer and leading dimension) wherever the column
    stride is 1. Anything else runs the reference's expression in torch."""
    rows = (user_emb, item_cf, item_kg)
    if any(not isinstance(x, torch.Tensor) or x.dim() != 2 for x in rows):
        return False
    d = int(user_emb.shape[1])
    params = [t for t in (W1, b1, W2) if t is not None]
    return (all(t.is_cuda and t.dtype == torch.float32 for t in (*rows, *params))
            and _width_ok(d, bool(params))
            and all(x.stride(1) != 1 or _rows_ok(x, d) for x in rows))


def _reference(user_emb, item_cf, item_kg, uid, pid, nid, reg, batch_size, W1, b1, W2):
    """The reference's expression in torch: the full fusion, the gathers, bpr_loss, l2_reg_loss
    and the division."""
    z = torch.stack([item_cf, item_kg], dim=1)
    if W1 is not None:
        w = F.linear(torch.tanh(F.linear(z, W1, b1)), W2)
        fused = (torch.softmax(w, dim=1) * z).sum(1)
    else:
        fused = torch.mean(z, dim=1)
    anc, pos, neg = user_emb[uid], fused[pid], fused[nid]
    x = (anc * pos).sum(dim=1) - (anc * neg).sum(dim=1)
    bpr = torch.mean(-torch.log(10e-6 + torch.sigmoid(x)))
    norms = torch.norm(anc, p=2) + torch.norm(pos, p=2) + torch.norm(neg, p=2)
    return bpr + norms * reg / batch_size


class _CFLoss(torch.autograd.Function):
    """hgd_cf_loss_forward / _backward. ``ids``: int32 [3, B] (uid, pid, nid)."""

    @staticmethod
    def forward(ctx, U, Z0, Z1, W1, b1, W2, ids, reg, bs, save):
        lib = nat.load()
        dev = U.device
        B, d = int(ids.shape[1]), int(U.shape[1])
        att = W1 is not None
        Uc, Z0c, Z1c = _rows(U), _rows(Z0), _rows(Z1)
        ps = [x.detach().contiguous() for x in (W1, b1, W2)] if att else [None] * 3
        f = dict(dtype=torch.float32, device=dev)
        beta0 = torch.empty((2 * B, d), **f) if att and save else None
        coef, norms, loss = torch.empty(B, **f), torch.empty(3, **f), torch.empty((), **f)
        wsb = lib.hgd_cf_loss_workspace_size(B, d, 0)
        ws = _ws(wsb, dev)
        ctx.call = (Uc.data_ptr(), _ld(Uc, d), ids[0].data_ptr(), int(U.shape[0]),
                    Z0c.data_ptr(), _ld(Z0c, d), Z1c.data_ptr(), _ld(Z1c, d), ids[1].data_ptr(),
                    ids[2].data_ptr(), int(Z0.shape[0]), B, d, *(nat.ptr(x) for x in ps), reg, bs)
        nat.check(lib.hgd_cf_loss_forward(*ctx.call, nat.ptr(beta0), d, coef.data_ptr(),
                                          norms.data_ptr(), loss.data_ptr(), ws.data_ptr(), wsb,
                                          _stream(dev)), "hgd_cf_loss_forward")
        if save:
            ctx.att, ctx.sizes = att, (int(U.shape[0]), int(Z0.shape[0]), B, d)
            # with what ctx.call points into, so that an in-place change before the backward is
            # caught
            ctx.save_for_backward(coef, norms, ids, Uc, Z0c, Z1c, *([beta0, *ps] if att else []))
        return loss

    @staticmethod
    def backward(ctx, g):
        coef, norms, ids = ctx.saved_tensors[:3]
        beta0 = ctx.saved_tensors[6] if ctx.att else None
        n_users, n_items, B, d = ctx.sizes
        need = ctx.needs_input_grad
        want_users, want_rows = need[0], need[1] or need[2]
        want_params = ctx.att and (need[3] or need[4] or need[5])
        out = [None] * 10
        if not (want_users or want_rows or want_params):
            return tuple(out)
        lib = nat.load()
        dev = coef.device
        f = dict(dtype=torch.float32, device=dev)
        g = g.detach().to(dtype=torch.float32).reshape(1).contiguous()
        DA = torch.empty((B, d), **f) if want_users else None
        D0 = D1 = None
        if want_rows:
            D0, D1 = torch.empty((2 * B, d), **f), torch.empty((2 * B, d), **f)
        dW1 = db1 = dW2 = ws = None
        wsb = 0
        if want_params:
            dW1, db1, dW2 = torch.empty((d, d), **f), torch.empty(d, **f), torch.empty((d, d), **f)
            wsb = lib.hgd_cf_loss_workspace_size(B, d, 1)
            ws = _ws(wsb, dev)
        nat.check(lib.hgd_cf_loss_backward(
            *ctx.call, nat.ptr(beta0), d, coef.data_ptr(), norms.data_ptr(), g.data_ptr(),
            nat.ptr(DA), d, nat.ptr(D0), d, nat.ptr(D1), d, nat.ptr(dW1), nat.ptr(db1),
            nat.ptr(dW2), nat.ptr(ws), wsb, _stream(dev)), "hgd_cf_loss_backward")
        if want_users:
            # dU = S·DA: user ← its triples, ascending
            out[0] = spmm_csr(scatter_csr(ids[0], n_users), DA)
        if want_rows:
            # item ← its positions among the 2B interleaved ones, ascending; one sort for both
            # views, one hop each (one hop over [DZ0 | DZ1] side by side measured slower, DESIGN
            # §4.12)
            csr = scatter_csr(torch.stack([ids[1], ids[2]], dim=1).reshape(-1), n_items)
            out[1] = spmm_csr(csr, D0) if need[1] else None
            out[2] = spmm_csr(csr, D1) if need[2] else None
        if want_params:
            out[3], out[4], out[5] = (dW1 if need[3] else None, db1 if need[4] else None,
                                      dW2 if need[5] else None)
        return tuple(out)


def _check(user_emb, item_cf, item_kg, uid, pid, nid, reg, batch_size, W1, b1, W2, what):
    """Every error of a call, before anything is launched; returns (B, d, reg, batch_size)."""
    params = ((W1, "W1"), (b1, "b1"), (W2, "W2"))
    given = [x is not None for x, _ in params]
    if any(given) and not all(given):
        raise ValueError(f"{what}: W1, b1 and W2 go together (all three for the attention, none "
                         f"for the mean of the views)")
    rows = ((user_emb, "user_emb"), (item_cf, "item_cf"), (item_kg, "item_kg"))
    for x, name in (*rows, *(params if all(given) else ())):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be a float32 tensor, got "
                            f"{getattr(x, 'dtype', type(x).__name__)}")
    for x, name in rows:
        if x.dim() != 2:
            raise ValueError(f"{what}: {name} must be [n, d], got {tuple(x.shape)}")
    d = int(user_emb.shape[1])
    if d == 0:
        raise ValueError(f"{what}: d must be > 0")
    if item_cf.shape != item_kg.shape:
        raise ValueError(f"{what}: item_cf {tuple(item_cf.shape)} and item_kg "
                         f"{tuple(item_kg.shape)} differ")
    if item_cf.shape[1] != d:
        raise ValueError(f"{what}: item_cf {tuple(item_cf.shape)} does not match d = {d}")
    if all(given):
        if tuple(W1.shape) != (d, d):
            raise ValueError(f"{what}: W1 {tuple(W1.shape)} does not match d = {d} (hidden_size "
                             f"must equal in_size)")
        if tuple(b1.shape) != (d,):
            raise ValueError(f"{what}: b1 {tuple(b1.shape)} does not match d = {d}")
        if tuple(W2.shape) != (d, d):
            raise ValueError(f"{what}: W2 {tuple(W2.shape)} does not match d = {d}")
    for x, name in ((uid, "uid"), (pid, "pid"), (nid, "nid")):
        _index_vector(x, name, what)
    B = int(uid.numel())
    if not (pid.numel() == nid.numel() == B):
        raise ValueError(f"{what}: uid, pid, nid differ in length ({B}, {pid.numel()}, "
                         f"{nid.numel()})")
    if B == 0:
        raise ValueError(f"{what}: an empty batch has no loss (the reference returns NaN)")
    if int(batch_size) <= 0:
        raise ValueError(f"{what}: batch_size must be > 0, got {batch_size}")
    n_users, n_items = int(user_emb.shape[0]), int(item_cf.shape[0])
    if n_users == 0 or n_items == 0 or max(n_users, n_items) >= 2 ** 31 - 1 or B >= 2 ** 30:
        raise ValueError(f"{what}: sizes must be in [1, 2^31 - 1) and B < 2^30")
    dev = user_emb.device
    for x, name in (*rows[1:], *(params if all(given) else ())):
        if x.device != dev:
            raise RuntimeError(f"{what}: {name} is on {x.device}, user_emb on {dev}")
    return B, d, float(reg), int(batch_size)


def cf_loss(user_emb: torch.Tensor, item_cf: torch.Tensor, item_kg: torch.Tensor,
            uid: torch.Tensor, pid: torch.Tensor, nid: torch.Tensor, reg: float, batch_size: int,
            W1: torch.Tensor = None, b1: torch.Tensor = None, W2: torch.Tensor = None,
            validate: bool = True, attention=None) -> torch.Tensor:
    """KHGRec.py:131-143 as a 0-dim loss: the fusion of ``item_cf`` / ``item_kg`` (``[n_items,
    d]``) at the rows ``pid`` / ``nid`` name, ``bpr_loss`` against ``user_emb[uid]`` and
    ``l2_reg_loss(reg, anchor, pos, neg) / batch_size``. ``batch_size`` is the configured
    ``self.batchSize`` the regulariser is divided by (the mean divides by the actual ``B``).

    ``W1``, ``b1``, ``W2``: the ``Attention`` parameters (``project[0].weight``, ``.bias``,
    ``project[2].weight``), all three or none; none is the reference's ``wo_attention`` mean of
    the two views. ``attention=``: a :class:`~.layers.Attention` instead of the three tensors.
    Gradients go to ``user_emb``, ``item_cf``, ``item_kg`` and the three parameters, each only
    when it requires one: a part that is not needed launches nothing. Inputs with unit column
    stride and 16-byte aligned rows (the halves of a stacked ``[n, 2, d]`` tensor, a column slice,
    the row blocks of one table) are read in place. ``validate``: read one error count back and
    raise ``ValueError`` on an id out of range; with ``validate=False`` nothing is read back and
    such an id is replaced by 0."""
    what = "cf_loss"
    if attention is not None:
        if W1 is not None or b1 is not None or W2 is not None:
            raise ValueError(f"{what}: give attention= or W1, b1, W2, not both")
        W1, b1, W2 = attention.weights()
    B, d, reg, bs = _check(user_emb, item_cf, item_kg, uid, pid, nid, reg, batch_size, W1, b1,
                           W2, what)
    if not cf_loss_supported(user_emb, item_cf, item_kg, W1, b1, W2):
        dev = user_emb.device
        return _reference(user_emb, item_cf, item_kg, uid.to(dev), pid.to(dev), nid.to(dev), reg,
                          bs, W1, b1, W2)
    dev = user_emb.device
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    n_users, n_items = int(user_emb.shape[0]), int(item_cf.shape[0])
    ids = torch.stack([_narrow(uid, n_users, flags, dev), _narrow(pid, n_items, flags, dev),
                       _narrow(nid, n_items, flags, dev)])
    if validate and int(flags.item()):
        raise ValueError(f"{what}: {int(flags.item())} ids out of range for {n_users} users / "
                         f"{n_items} items")
    tensors = [t for t in (user_emb, item_cf, item_kg, W1, b1, W2) if t is not None]
    save = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    return _CFLoss.apply(user_emb, item_cf, item_kg, W1, b1, W2, ids, reg, bs, save)
