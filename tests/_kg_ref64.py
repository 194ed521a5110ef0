"""Float64 CPU restatements of KHGRec's KG attention (model/graph/KHGRec.py:298-331, :419-453)
with the reference's own torch calls, and the test graph the KG-attention tests share."""
import numpy as np
import torch

N_ENT, N_REL, B = 97, 5, 300


def graph(seed=0):
    """300 triples over 97 entities and 5 relations, shuffled, containing: an empty relation (4),
    a relation with a single triple (3), a pair repeated under one relation ((10, 20) twice under
    0), a pair repeated under two relations ((11, 21) under 0 and 1), heads with exactly one
    triple (12 and 14), a head all of whose triples are one duplicate group ((13, 30) three
    times), and head 0 holding 200 of the 300 triples. Returns int64 tensors (h, t, r)."""
    rng = np.random.default_rng(seed)
    fixed = [(10, 20, 0), (10, 20, 0), (11, 21, 0), (11, 21, 1), (12, 22, 2),
             (13, 30, 0), (13, 30, 1), (13, 30, 0), (14, 40, 3)]
    big = [(0, int(rng.integers(0, N_ENT)), int(rng.integers(0, 3))) for _ in range(200)]
    rest = [(int(rng.integers(15, N_ENT)), int(rng.integers(0, N_ENT)), int(rng.integers(0, 3)))
            for _ in range(B - 200 - len(fixed))]
    tri = np.array(fixed + big + rest, dtype=np.int64)[rng.permutation(B)]
    assert tri.shape == (B, 3)
    return tuple(torch.from_numpy(np.ascontiguousarray(tri[:, k])) for k in range(3))


def one_head(n, seed=1, head=5):
    """n triples that all share one head (a row as long as the batch)."""
    rng = np.random.default_rng(seed)
    return (torch.full((n,), head, dtype=torch.int64),
            torch.from_numpy(rng.integers(0, N_ENT, n)), torch.from_numpy(rng.integers(0, 3, n)))


def tables(d, dr, seed=0, n_ent=N_ENT, n_rel=N_REL):
    """(E, trans_M, relation_emb) in fp32: xavier-uniform parameters (KHGRec.py:256-257) and a
    normal table scaled so that a projection (E·W_r)_k has variance 1/2 at every width, which
    puts the scores at |s| = O(1-10)."""
    g = torch.Generator().manual_seed(seed)
    E = torch.randn(n_ent, d, generator=g) * ((d + dr) / (4.0 * d)) ** 0.5
    W = (torch.rand(n_rel, d, dr, generator=g) * 2 - 1) * (6.0 / (d + dr)) ** 0.5
    R = (torch.rand(n_rel, dr, generator=g) * 2 - 1) * (6.0 / (n_rel + dr)) ** 0.5
    return E, W, R


def scores(E, W, R, h, t, r, relations):
    """update_attention's per-relation loop (KHGRec.py:312-324) in float64. Returns the
    concatenated (rows, cols, values, mag, index): ``index`` the batch position of every entry,
    ``mag`` = Σ_k (|E[t]|·|W_r|)_k·(1 + (|E[h]|·|W_r|)_k + |R[r]_k|), the sum of the absolute
    terms behind a score (tanh has slope <= 1)."""
    E, W, R = E.double(), W.double(), R.double()
    rows, cols, vals, mags, index = [], [], [], [], []
    for r_idx in relations:
        (idx,) = torch.where(r == r_idx)
        bh, bt = h[idx], t[idx]
        W_r, r_embed = W[r_idx], R[r_idx]
        r_mul_h = torch.matmul(E[bh], W_r)
        r_mul_t = torch.matmul(E[bt], W_r)
        vals.append(torch.sum(r_mul_t * torch.tanh(r_mul_h + r_embed), dim=1))
        a_h = torch.matmul(E[bh].abs(), W_r.abs())
        a_t = torch.matmul(E[bt].abs(), W_r.abs())
        mags.append(torch.sum(a_t * (1 + a_h + r_embed.abs()), dim=1))
        rows.append(bh)
        cols.append(bt)
        index.append(idx)
    return tuple(torch.cat(x) for x in (rows, cols, vals, mags, index))


def sparse_softmax_dense(rows, cols, vals, n):
    """torch.sparse.softmax(A_in.cpu(), dim=1) (KHGRec.py:326-330) of the uncoalesced COO, as a
    dense float64 [n, n] (unspecified entries 0)."""
    A = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals.double(), (n, n))
    return torch.sparse.softmax(A, dim=1).to_dense()


def update_attention(E, W, R, h, t, r, relations, n):
    """update_attention in float64: (dense softmax [n, n], dense Σ score magnitude per (h, t))."""
    rows, cols, vals, mag, _ = scores(E, W, R, h, t, r, relations)
    G = torch.zeros(n, n, dtype=torch.float64).index_put_((rows, cols), mag, accumulate=True)
    return sparse_softmax_dense(rows, cols, vals, n), G


def dense_of(inc):
    """An attention Incidence coalesced on the host: float32 [n_rows, n_cols] (a run's value plus
    exact zeros, so the sum is exact). The row pointers may end before the arrays do."""
    rp = inc.csr.rowptr.cpu()
    live = int(rp[-1])
    rows = torch.repeat_interleave(torch.arange(inc.n_rows), rp[1:] - rp[:-1])
    out = torch.zeros(inc.n_rows, inc.n_cols)
    out.index_put_((rows, inc.csr.col.cpu().long()[:live]), inc.val.cpu()[:live], accumulate=True)
    return out


def dense_of_t(inc):
    """The same matrix from the CSC side (``val_t``)."""
    cp = inc.csc.rowptr.cpu()
    live = int(cp[-1])
    cols = torch.repeat_interleave(torch.arange(inc.n_cols), cp[1:] - cp[:-1])
    out = torch.zeros(inc.n_rows, inc.n_cols)
    out.index_put_((inc.csc.col.cpu().long()[:live], cols), inc.val_t.cpu()[:live],
                   accumulate=True)
    return out


def att_conv(att, K, x, act, slope):
    """AttHGCNConv.forward (KHGRec.py:445-453) on dense float64 matrices."""
    adj = att @ K
    y = adj @ (adj.t() @ x)
    return torch.nn.functional.leaky_relu(y, slope) if act else y


def relational_encoder(lns, att, K, x, slope):
    """RelationalAwareEncoder.forward (KHGRec.py:431-438) with float64 LayerNorms ``lns``."""
    res = x
    L = len(lns)
    for i, ln in enumerate(lns):
        y = att_conv(att, K, x, act=i != L - 1, slope=slope)
        x = torch.nn.functional.layer_norm(y, (y.shape[1],), ln.weight, ln.bias, ln.eps) + res
    return x
