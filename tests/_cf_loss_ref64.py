"""Float64 CPU restatement of KHGRec's CF loss block (model/graph/KHGRec.py:131-143 and
calculate_cf_loss, :341-345) with the reference's own torch calls and autograd, the magnitude
surrogate the CF-loss tests bound their errors with, and the tests' inputs. Builds on
tests/_view_attention_ref64.py (``attention``, ``surrogate``, ``inputs``).

The surrogate takes c_k = σ(x_k)(1 − σ(x_k))/(1e-5 + σ(x_k)) from the float64 run as constants
and replaces every table by its absolute value:
    O   = surrogate(|z0|, |z1|, …)[0]            (mean mode: (|z0| + |z1|)/2)
    X_k = Σ_j |a_kj| · (O_2k,j + O_2k+1,j)       (positions interleaved: 2k positive, 2k+1 negative)
    R   = reg · (‖|A|‖ + ‖O_P‖ + ‖O_N‖) / batch_size
``mag`` of every gradient is the float64 autograd of mean_k(c_k·X_k) + R with respect to the
absolute tables; mag(loss) = mean_k(ℓ_k + X_k) + R. It is NOT valid for saturated scores (c_k → 0:
the reference's own fp32 gradients are then 1e-2·mag off float64)."""
import torch

from tests import _view_attention_ref64 as V

N_ITEMS, N_USERS, N_POS = 300, 40, 30
GRADS = ("dU", "dZ0", "dZ1", "dW1", "db1", "dW2")


def inputs(B, d, seed=0, user_scale=0.1, n_items=N_ITEMS, n_users=N_USERS):
    """The standard inputs: dict(users, z0, z1, W1, b1, W2, uid, pid, nid). Items from
    _view_attention_ref64.inputs(n_items, d) (every 7th row has z1 == z0), users = user_scale ·
    N(0, 1), uid over all users, pid over the first 30 items (repeats), nid over all items with
    nid[::5] = pid[::5] (x_k = 0 exactly; an item both positive and negative) — except B = 1,
    where nid != pid."""
    z0, z1, W1, b1, W2, _ = V.inputs(n_items, d)
    gen = torch.Generator().manual_seed(77000 + 1000 * seed + 13 * d + B)
    users = user_scale * torch.randn(n_users, d, generator=gen)
    uid = torch.randint(0, n_users, (B,), generator=gen)
    pid = torch.randint(0, N_POS, (B,), generator=gen)
    nid = torch.randint(0, n_items, (B,), generator=gen)
    if B > 1:
        nid[::5] = pid[::5]
    elif nid[0] == pid[0]:
        nid[0] = (pid[0] + 1) % n_items
    return dict(users=users, z0=z0, z1=z1, W1=W1, b1=b1, W2=W2, uid=uid, pid=pid, nid=nid)


def cf_loss(users, z0, z1, uid, pid, nid, reg, batch_size, params):
    """The reference's ops (any dtype): the full fusion, the gathers, bpr_loss, l2_reg_loss / the
    configured batch size. Returns (loss, x) with x the score differences."""
    z = torch.stack([z0, z1], dim=1)
    fused = V.attention(z, *params)[0] if params is not None else torch.mean(z, dim=1)
    anc, pos, neg = users[uid], fused[pid], fused[nid]
    x = torch.mul(anc, pos).sum(dim=1) - torch.mul(anc, neg).sum(dim=1)
    bpr = torch.mean(-torch.log(10e-6 + torch.sigmoid(x)))
    emb = torch.norm(anc, p=2) + torch.norm(pos, p=2) + torch.norm(neg, p=2)
    return bpr + emb * reg / batch_size, x


def reference(inp, reg, batch_size, attention=True):
    """(ref, mag): float64 loss and the gradients GRADS (the parameters' only with attention),
    and the surrogate's values of the same names; ref also holds ``coef`` (c_k)."""
    names = ("users", "z0", "z1") + (("W1", "b1", "W2") if attention else ())
    uid, pid, nid = inp["uid"], inp["pid"], inp["nid"]
    leaves = [inp[k].double().clone().requires_grad_(True) for k in names]
    loss, x = cf_loss(*leaves[:3], uid, pid, nid, reg, batch_size,
                      leaves[3:] if attention else None)
    grads = torch.autograd.grad(loss, leaves)
    ref = dict(loss=loss.detach(), **dict(zip(GRADS, grads)))
    s = torch.sigmoid(x.detach())
    ell = -torch.log(10e-6 + s)
    c = s * (1 - s) / (10e-6 + s)
    ref["coef"] = c
    al = [inp[k].double().abs().clone().requires_grad_(True) for k in names]
    if attention:
        O = V.surrogate(torch.stack(al[1:3], dim=1), *al[3:])[0]
    else:
        O = (al[1] + al[2]) / 2
    A, OP, ON = al[0][uid], O[pid], O[nid]
    X = (A * (OP + ON)).sum(dim=1)
    Rg = reg * (torch.norm(A, p=2) + torch.norm(OP, p=2) + torch.norm(ON, p=2)) / batch_size
    mgrads = torch.autograd.grad((c * X).mean() + Rg, al)
    mag = dict(loss=((ell + X).mean() + Rg).detach(), **dict(zip(GRADS, mgrads)))
    return ref, mag
