"""Float64 CPU restatement of KHGRec's calculate_kg_loss (model/graph/KHGRec.py:347-365) with the
reference's own torch calls and autograd, and the magnitude surrogate the KG-loss tests bound
their errors with. The graph and the tables are those of tests/_kg_ref64.py."""
import torch
import torch.nn.functional as F

from tests import _kg_ref64 as K

REG_KG = 0.5      # large enough that the regulariser's gradient stands above the bound
BATCH_SIZE_KG = 256  # the configured size the regulariser divides by; never the tests' B


def neg_tails(pos_t, n_ent=K.N_ENT, seed=5):
    """Sampled negative tails: torch.randint with a fixed generator, every 7th equal to the
    positive tail (a triple whose two scores are bitwise equal)."""
    g = torch.Generator().manual_seed(seed)
    neg = torch.randint(0, n_ent, (len(pos_t),), generator=g)
    neg[::7] = pos_t[::7]
    return neg


def calculate_kg_loss(x_h, r, x_p, x_n, trans_M, relation_emb, reg_kg, batch_size_kg,
                      surrogate=False):
    """What KHGRec.py:347-365 computes, with its torch calls in its order: the two parameter
    gathers, three torch.bmm, the squared distances, −logsigmoid(neg − pos), the mean, and
    l2_reg_loss (util/loss_torch.py:17-21: the sum of the four torch.norm, times reg) divided by
    the configured batch size. ``surrogate``: the same expression with both differences
    replaced by sums and softplus replaced by (pos + neg) — over absolute tables it is the sum
    of the absolute terms behind the loss, and its autograd that behind every gradient."""
    e = relation_emb[r]
    W_r = trans_M[r]
    a, p, n = (torch.bmm(x.unsqueeze(1), W_r).squeeze(1) for x in (x_h, x_p, x_n))
    if surrogate:
        pos = torch.sum(torch.pow(a + e + p, 2), dim=1)
        neg = torch.sum(torch.pow(a + e + n, 2), dim=1)
        per_triple = pos + neg
    else:
        pos = torch.sum(torch.pow(a + e - p, 2), dim=1)
        neg = torch.sum(torch.pow(a + e - n, 2), dim=1)
        per_triple = (-1.0) * F.logsigmoid(neg - pos)
    norms = sum(torch.norm(x, p=2) for x in (a, e, p, n))
    return torch.mean(per_triple) + norms * reg_kg / batch_size_kg, (pos - neg).detach()


def _one(E, W, R, h, pos_t, neg_t, r, reg_kg, batch_size_kg, surrogate):
    E, W, R = (x.detach().clone().requires_grad_(True) for x in (E, W, R))
    rows = [E[i] for i in (h, pos_t, neg_t)]
    for x in rows:
        x.retain_grad()
    loss, diff = calculate_kg_loss(rows[0], r, rows[1], rows[2], W, R, reg_kg, batch_size_kg,
                                   surrogate)
    loss.backward()
    return dict(loss=loss.detach(), dE=E.grad, dW=W.grad, dR=R.grad, diff=diff,
                rows=[x.grad for x in rows])


def reference(E, W, R, h, pos_t, neg_t, r, reg_kg=REG_KG, batch_size_kg=BATCH_SIZE_KG):
    """(ref, mag): float64 loss and gradients (dE, dW, dR, the three row gradients, and the
    per-triple score difference pos − neg), and the surrogate's values of the same names."""
    E, W, R = E.double(), W.double(), R.double()
    ref = _one(E, W, R, h, pos_t, neg_t, r, reg_kg, batch_size_kg, False)
    mag = _one(E.abs(), W.abs(), R.abs(), h, pos_t, neg_t, r, reg_kg, batch_size_kg, True)
    return ref, mag
