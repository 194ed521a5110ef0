"""Float64 CPU restatement of KHGRec's view fusion (Attention.forward, model/graph/KHGRec.py:
466-480) with the reference's own torch calls and autograd, the magnitude surrogate the
view-attention tests bound their errors with, and the tests' inputs.

The surrogate runs over absolute tables and |dOut| with every difference a sum. With A_v the
surrogate of the pre-activation:
    A_v = |z_v|·|W1|ᵀ + |b1|,  T_v = A_v (tanh is 1-Lipschitz),  Q = (T_0 + T_1)·|W2|ᵀ,
    O = (|z0| + |z1|) ⊙ (1 + Q/4)   (σ′ <= 1/4)
``mag`` of every gradient is the surrogate's autograd; of β0 it is Q/4 (an absolute bound)."""
import math

import torch
import torch.nn.functional as F


def inputs(N, d, s=1.0, seed=0, w2_scale=1.0):
    """(z0, z1, W1, b1, W2, g) float32: weights uniform ±√(6/2d), b1 uniform ±1/√d,
    z ~ N(0, s²), dOut ~ N(0, 1); every 7th row has z1 == z0 bitwise."""
    gen = torch.Generator().manual_seed(1000 * seed + d)
    a = math.sqrt(6.0 / (2 * d))
    W1 = (torch.rand(d, d, generator=gen) * 2 - 1) * a
    b1 = (torch.rand(d, generator=gen) * 2 - 1) / math.sqrt(d)
    W2 = (torch.rand(d, d, generator=gen) * 2 - 1) * a * w2_scale
    gen = torch.Generator().manual_seed(1000 * seed + 7 * d + N)
    z0 = torch.randn(N, d, generator=gen) * s
    z1 = torch.randn(N, d, generator=gen) * s
    z1[::7] = z0[::7]
    g = torch.randn(N, d, generator=gen)
    return z0, z1, W1, b1, W2, g


def attention(z, W1, b1, W2):
    """Attention.forward on the stacked [N, 2, d] tensor: project, softmax over the views, sum."""
    w = F.linear(torch.tanh(F.linear(z, W1, b1)), W2)
    beta = torch.softmax(w, dim=1)
    return (beta * z).sum(1), beta


def surrogate(z, W1, b1, W2):
    """(O, Q) over absolute tables."""
    T = F.linear(z, W1, b1)
    Q = F.linear(T[:, 0] + T[:, 1], W2)
    return (z[:, 0] + z[:, 1]) * (1 + Q / 4), Q


def _grads(out, leaves, g):
    got = torch.autograd.grad(out, leaves, g, allow_unused=True)
    return dict(zip(("dz0", "dz1", "dW1", "db1", "dW2"), got))


def reference(z0, z1, W1, b1, W2, g=None, upstream=None):
    """(ref, mag): float64 out, beta0 and the five gradients, and the surrogate's values of the
    same names. ``g``: dOut. ``upstream(out) -> (dOut, |dOut| surrogate)`` instead: a loss chained
    behind ``out`` (its float64 gradient and that gradient's magnitude)."""
    leaves = [x.double().clone().requires_grad_(True) for x in (z0, z1, W1, b1, W2)]
    out, beta = attention(torch.stack(leaves[:2], dim=1), *leaves[2:])
    if upstream is not None:
        g, gmag = upstream(out)
    else:
        g = g.double()
        gmag = g.abs()
    ref = dict(out=out.detach(), beta0=beta[:, 0].detach(), **_grads(out, leaves, g))
    al = [x.double().abs().clone().requires_grad_(True) for x in (z0, z1, W1, b1, W2)]
    O, Q = surrogate(torch.stack(al[:2], dim=1), *al[2:])
    mag = dict(out=O.detach(), beta0=Q.detach() / 4, **_grads(O, al, gmag))
    return ref, mag
