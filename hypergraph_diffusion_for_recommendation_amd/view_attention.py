"""KHGRec's view fusion on the device (model/graph/KHGRec.py:466-480, called at :132 and :202).

The reference fuses an item's collaborative and knowledge-graph views with ::

    item_emb_fused, _ = self.attention_item(torch.stack([item_emb_cf, item_emb_kg], dim=1))

where ``Attention`` is ``Linear(d, d) → Tanh → Linear(d, d, bias=False)`` on both views, a softmax
over the two views per (row, channel) and the weighted sum: one ``[N, 2, d]`` stack copy, about
eight kernels forward and twice that backward, five ``[N, 2, d]`` intermediates. Here the forward
is one kernel that reads the two views and writes ``out`` (and ``β0 [N, d]`` when a backward will
follow), and the backward is one kernel that recomputes the two ``tanh`` rows and writes both row
gradients (``hgd_view_attention_forward`` / ``_backward``). With two views the softmax is
``β0 = σ((t_0 − t_1)·W2ᵀ)``: three products per row forward, not four.

* :func:`view_attention` takes the two views as separate ``[N, d]`` tensors (or strided views of
  wider ones): no ``torch.stack``.
* :func:`view_attention_stacked` takes the reference's ``[N, 2, d]`` tensor, reads its halves in
  place and returns its gradient as one ``[N, 2, d]`` tensor (:class:`~.layers.Attention`).
* :func:`view_attention_supported` says which path a call takes: widths outside the fused set,
  unaligned views and CPU tensors run the reference's own expression in torch.

fp32, deterministic (every sum in a fixed order, no float atomics), a row's results independent
of ``N`` and of its position. ``beta`` as a returned value is non-differentiable: every caller in
the reference discards it (``item_emb_fused, _ = …``). Nothing is read back from the device and
every buffer comes from torch's allocator on the current stream, so a call can sit inside a
captured step.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _native as nat
from .incidence import _stream, _ws

__all__ = ["view_attention", "view_attention_stacked", "view_attention_supported", "ROW_BLOCK"]



def __getattr__(name):
    """``ROW_BLOCK``: the rows of one workgroup, read from the library
    (``hgd_view_attention_row_block``) so that there is one source for it."""
    if name == "ROW_BLOCK":
        return int(nat.load().hgd_view_attention_row_block())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _check(z0, z1, weight1, bias1, weight2, what: str, names=("z0", "z1")):
    """dtype, rank, shape and device checks; returns (N, d)."""
    args = ((z0, names[0]), (z1, names[1]), (weight1, "weight1"), (bias1, "bias1"),
            (weight2, "weight2"))
    for x, name in args:
        if x is None and name == names[1]:
            continue
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be a float32 tensor, got "
                            f"{getattr(x, 'dtype', type(x).__name__)}")
    if z1 is None:  # the stacked form
        if z0.dim() != 3 or z0.shape[1] != 2:
            raise ValueError(f"{what}: {names[0]} must be [N, 2, d] (two stacked views), got "
                             f"{tuple(z0.shape)}")
        N, d = int(z0.shape[0]), int(z0.shape[2])
    else:
        if z0.dim() != 2 or z1.dim() != 2:
            raise ValueError(f"{what}: z0 and z1 must be [N, d], got {tuple(z0.shape)}, "
                             f"{tuple(z1.shape)}")
        if z0.shape != z1.shape:
            raise ValueError(f"{what}: z0 {tuple(z0.shape)} and z1 {tuple(z1.shape)} differ")
        N, d = int(z0.shape[0]), int(z0.shape[1])
    if d == 0:
        raise ValueError(f"{what}: d must be > 0")
    if weight1.dim() != 2 or weight1.shape[1] != d:
        raise ValueError(f"{what}: weight1 {tuple(weight1.shape)} does not match d = {d}")
    if weight1.shape[0] != d:
        raise ValueError(f"{what}: weight1 {tuple(weight1.shape)}: hidden_size must equal "
                         f"in_size = {d} (the reference's beta * z broadcast needs it)")
    if tuple(bias1.shape) != (d,):
        raise ValueError(f"{what}: bias1 {tuple(bias1.shape)} does not match d = {d}")
    if tuple(weight2.shape) != (d, d):
        raise ValueError(f"{what}: weight2 {tuple(weight2.shape)} does not match d = {d}")
    dev = z0.device
    for x, name in args[1:]:
        if x is not None and x.device != dev:
            raise RuntimeError(f"{what}: {name} is on {x.device}, {names[0]} on {dev}")
    return N, d


def _rows_ok(x: torch.Tensor, d: int) -> bool:
    """A [N, d] view the kernels read or write in place: unit column stride, 16-byte aligned
    rows."""
    return (x.stride(1) == 1 and (x.shape[0] <= 1 or (x.stride(0) >= d and x.stride(0) % 4 == 0))
            and x.data_ptr() % 16 == 0)


def _ld(x: torch.Tensor, d: int) -> int:
    return x.stride(0) if x.shape[0] > 1 else d


def view_attention_supported(z0: torch.Tensor, z1: torch.Tensor = None, weight1=None,
                             bias1=None, weight2=None) -> bool:
    """True when a call with these arguments runs the fused kernels: device float32 tensors, a
    width that is a multiple of 16 in [16, 128], and views with 16-byte aligned rows (pointer and
    leading dimension). ``z1`` None: ``z0`` is the stacked ``[N, 2, d]`` tensor. Anything else
    runs the reference's expression in torch."""
    views = (z0[:, 0], z0[:, 1]) if z1 is None and z0.dim() == 3 else (z0, z1)
    if any(v is None or v.dim() != 2 for v in views):
        return False
    d = int(views[0].shape[1])
    tensors = [t for t in (*views, weight1, bias1, weight2) if t is not None]
    return (all(t.is_cuda and t.dtype == torch.float32 for t in tensors)
            and d % 16 == 0 and 16 <= d <= 128 and views[0].shape[0] < 2 ** 40
            and all(_rows_ok(v, d) for v in views))


def _reference(z, weight1, bias1, weight2):
    """Attention.forward (KHGRec.py:477-480) on the stacked [N, 2, d] tensor, in torch."""
    w = F.linear(torch.tanh(F.linear(z, weight1, bias1)), weight2)
    beta = torch.softmax(w, dim=1)
    return (beta * z).sum(1), beta


class _ViewAttention(torch.autograd.Function):
    """hgd_view_attention_forward / _backward. ``z1`` None: ``z0`` is the stacked [N, 2, d]
    tensor, whose halves are read in place and whose gradient is written as one tensor."""

    @staticmethod
    def forward(ctx, z0, z1, W1, b1, W2, save_beta0):
        lib = nat.load()
        dev = z0.device
        stacked = z1 is None
        zs = z0.detach()
        v0, v1 = (zs[:, 0], zs[:, 1]) if stacked else (zs, z1.detach())
        N, d = v0.shape
        W1c, b1c, W2c = (x.detach().contiguous() for x in (W1, b1, W2))
        f = dict(dtype=torch.float32, device=dev)
        out = torch.empty((N, d), **f)
        beta0 = torch.empty((N, d), **f) if save_beta0 else None
        if N > 0:
            nat.check(lib.hgd_view_attention_forward(
                v0.data_ptr(), _ld(v0, d), v1.data_ptr(), _ld(v1, d), N, d, W1c.data_ptr(),
                b1c.data_ptr(), W2c.data_ptr(), out.data_ptr(), d, nat.ptr(beta0), d,
                _stream(dev)), "hgd_view_attention_forward")
        ctx.stacked = stacked
        # β0 is an output without a gradient: no zeros tensor is made for it in the backward
        ctx.set_materialize_grads(False)
        if save_beta0:
            # t_v is not saved: the backward recomputes it from the views
            ctx.save_for_backward(zs, None if stacked else v1, beta0, W1c, b1c, W2c)
            ctx.mark_non_differentiable(beta0)
        return out, beta0

    @staticmethod
    def backward(ctx, g, _g_beta0=None):
        if g is None:
            return None, None, None, None, None, None
        zs, v1, beta0, W1c, b1c, W2c = ctx.saved_tensors
        lib = nat.load()
        dev = zs.device
        v0, v1 = (zs[:, 0], zs[:, 1]) if ctx.stacked else (zs, v1)
        N, d = v0.shape
        need = ctx.needs_input_grad
        want_rows = need[0] or need[1]
        want_params = need[2] or need[3] or need[4]
        f = dict(dtype=torch.float32, device=dev)
        dz = d0 = d1 = dW1 = db1 = dW2 = None
        if want_rows:
            if ctx.stacked:
                dz = torch.empty((N, 2, d), **f)
                d0, d1 = dz[:, 0], dz[:, 1]
            else:
                d0, d1 = torch.empty((N, d), **f), torch.empty((N, d), **f)
        if want_params:
            alloc = torch.empty if N > 0 else torch.zeros
            dW1, db1, dW2 = alloc((d, d), **f), alloc((d,), **f), alloc((d, d), **f)
        if N > 0 and (want_rows or want_params):
            g = g.detach()
            if g.dtype != torch.float32 or not _rows_ok(g, d):
                g = g.to(torch.float32).contiguous()
            wsb = (lib.hgd_view_attention_workspace_size(N, d, _ld(v0, d), _ld(v1, d))
                   if want_params else 0)
            ws = _ws(wsb, dev) if want_params else None
            nat.check(lib.hgd_view_attention_backward(
                v0.data_ptr(), _ld(v0, d), v1.data_ptr(), _ld(v1, d), N, d, W1c.data_ptr(),
                b1c.data_ptr(), W2c.data_ptr(), beta0.data_ptr(), d, g.data_ptr(), _ld(g, d),
                nat.ptr(d0), _ld(d0, d) if want_rows else 0, nat.ptr(d1),
                _ld(d1, d) if want_rows else 0, nat.ptr(dW1), nat.ptr(db1), nat.ptr(dW2),
                nat.ptr(ws), wsb, _stream(dev)), "hgd_view_attention_backward")
        if ctx.stacked:
            gz0, gz1 = (dz if need[0] else None), None
        else:
            gz0, gz1 = (d0 if need[0] else None), (d1 if need[1] else None)
        return (gz0, gz1, dW1 if need[2] else None, db1 if need[3] else None,
                dW2 if need[4] else None, None)


def _fused(z0, z1, weight1, bias1, weight2, return_beta: bool):
    tensors = [t for t in (z0, z1, weight1, bias1, weight2) if t is not None]
    grad = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    out, beta0 = _ViewAttention.apply(z0, z1, weight1, bias1, weight2, grad or return_beta)
    if not return_beta:
        return out
    return out, torch.stack([beta0, 1.0 - beta0], dim=1)


def view_attention(z0: torch.Tensor, z1: torch.Tensor, weight1: torch.Tensor,
                   bias1: torch.Tensor, weight2: torch.Tensor, *, return_beta: bool = False):
    """``Attention.forward(torch.stack([z0, z1], dim=1))`` (KHGRec.py:466-480; the call sites
    :132 and :202 pass ``item_emb_cf`` and ``item_emb_kg``) without the stack: ``z0``, ``z1``
    are ``[N, d]`` (strided views with 16-byte aligned rows are read in place), ``weight1``,
    ``bias1`` are ``project[0]``'s and ``weight2`` is ``project[2].weight``, all ``[d, d]`` /
    ``[d]`` (``hidden_size == in_size``, which the reference's ``beta * z`` needs).

    Returns ``out [N, d]``; with ``return_beta=True`` also ``beta [N, 2, d]``, the softmax over
    the two views, which is NOT differentiable here (the reference's callers discard it).
    Gradients go to both views and to the three parameters, each only when it requires one: with
    the parameters frozen the backward is one kernel that stores nothing but the two row
    gradients. ``N = 0`` returns empty tensors (zero parameter gradients) and launches nothing."""
    what = "view_attention"
    _check(z0, z1, weight1, bias1, weight2, what)
    if view_attention_supported(z0, z1, weight1, bias1, weight2):
        return _fused(z0, z1, weight1, bias1, weight2, return_beta)
    out, beta = _reference(torch.stack([z0, z1], dim=1), weight1, bias1, weight2)
    return (out, beta.detach()) if return_beta else out


def view_attention_stacked(z: torch.Tensor, weight1: torch.Tensor, bias1: torch.Tensor,
                           weight2: torch.Tensor, *, return_beta: bool = False):
    """:func:`view_attention` on the reference's stacked ``[N, 2, d]`` tensor: its two halves are
    read in place (leading dimension 2d) and its gradient comes back as one ``[N, 2, d]``
    tensor."""
    what = "view_attention_stacked"
    _check(z, None, weight1, bias1, weight2, what, names=("z", None))
    if view_attention_supported(z, None, weight1, bias1, weight2):
        return _fused(z, None, weight1, bias1, weight2, return_beta)
    out, beta = _reference(z, weight1, bias1, weight2)
    return (out, beta.detach()) if return_beta else out
