"""A numpy float64 restatement of the fused BPR loss (csrc/bpr.hip), independent of its structure.

    anc = E[uid], pos = E[nu + pid], neg = E[nu + nid]          (E = [users ; items], [nu + ni, d])
    s_k = <anc_k, pos_k> - <anc_k, neg_k>
    term_k = -log(1e-5 + sigmoid(s_k)),  loss = mean_k term_k
    d loss / d s_k = -coef_k / B,  coef = sigmoid (1 - sigmoid) / (1e-5 + sigmoid)

Ids follow torch indexing where torch accepts them (negatives wrap); the library clamps what torch
refuses and counts the batch rows that held such an id (:func:`resolve`). The backward is three
``np.add.at`` scatters; nothing here knows of lane groups, lists, windows or heavy rows.
tests/test_bpr_ref.py checks this file against torch's float64 autograd.

:func:`exact_case` draws data on which every float32 product and every partial sum of the kernels
is exact, whatever the order and with or without fused multiply-adds, so a device result can be
compared with ``==``.
"""
from types import SimpleNamespace

import numpy as np

EPS = 1e-5  # the reference's 10e-6 (util/loss_torch.py:8)


def resolve(ids, n):
    """``(rows, bad)``: the table row each id names in a block of ``n`` rows and whether torch
    would have refused it. Ids in [-n, n) resolve as torch does; below -n clamps to row 0, at or
    above n to row n - 1 (Python integers: no int64 wrap-around at the extremes)."""
    rows, bad = [], []
    for i in np.asarray(ids).reshape(-1).tolist():
        ok = -n <= i < n
        rows.append((i + n if i < 0 else i) if ok else (0 if i < 0 else n - 1))
        bad.append(not ok)
    return np.array(rows, dtype=np.int64), np.array(bad, dtype=bool)


def _rows(nu, ni, uid, pid, nid):
    ru, bu = resolve(uid, nu)
    rp, bp = resolve(pid, ni)
    rn, bn = resolve(nid, ni)
    return ru, nu + rp, nu + rn, bu | bp | bn


def forward(E, nu, ni, uid, pid, nid):
    E = np.asarray(E, dtype=np.float64)
    ru, rp, rn, bad = _rows(nu, ni, uid, pid, nid)
    anc, pos, neg = E[ru], E[rp], E[rn]
    s = (anc * pos).sum(1) - (anc * neg).sum(1)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-s))
        one_minus = 1.0 / (1.0 + np.exp(s))  # 1 - sigmoid without the cancellation
    term = -np.log(EPS + sig)
    coef = sig * one_minus / (EPS + sig)
    loss = term.mean() if term.size else np.float64("nan")
    return SimpleNamespace(anc=anc, pos=pos, s=s, term=term, coef=coef, loss=loss,
                           bad_rows=int(bad.sum()))


def backward(E, nu, ni, uid, pid, nid, coef, grad):
    """``(dE, mag)`` [nu + ni, d]: the table gradient of ``grad · loss`` given the rows' ``coef``,
    and the same chain on absolute values (the sum of the magnitudes of each entry's terms)."""
    E = np.asarray(E, dtype=np.float64)
    ru, rp, rn, _ = _rows(nu, ni, uid, pid, nid)
    B = ru.size
    t = (-float(grad) * np.asarray(coef, dtype=np.float64) / B)[:, None]
    anc, pos, neg = E[ru], E[rp], E[rn]
    dE, mag = np.zeros_like(E), np.zeros_like(E)
    np.add.at(dE, ru, t * (pos - neg))
    np.add.at(dE, rp, t * anc)
    np.add.at(dE, rn, -t * anc)
    np.add.at(mag, ru, np.abs(t) * (np.abs(pos) + np.abs(neg)))
    np.add.at(mag, rp, np.abs(t) * np.abs(anc))
    np.add.at(mag, rn, np.abs(t) * np.abs(anc))
    return dE, mag


def exact_case(rng, nu, ni, d, uid, pid, nid, m=0, sign=None):
    """Data for the batch (uid, pid, nid) on which float32 arithmetic is exact in any order.

    E entries are drawn from {-4 .. 4}/4, coef from {0 .. 8}/8 and grad = ±B·2^m, so -grad/B is
    the power of two ∓2^m (B < 2^24: the quotient is exact). Then t = (-grad/B)·coef is a multiple
    of 2^(m-3), pos - neg a multiple of 1/4 with magnitude at most 2, every product a multiple of
    the unit 2^(m-5), and a product of the forward's dots a multiple of 1/16. A partial sum, in
    whatever order and grouping, is bounded by the sum of the magnitudes of its terms; asserted
    below to stay under 2^24 units (with at most 15,000 terms of at most 2^6 units it is under
    2^20), it is an integer number of units that float32 holds exactly. A fused multiply-add
    rounds the exact product plus the addend, which is again that exact sum. Asserted as well:
    the float64 gradient and dots survive the round trip through float32.

    Returns E, the int64 ids, coef, grad (float32 [1]) and the references: ``anc``, ``pos``
    (float32), ``s`` (float64, exact), ``dE`` (float32, == the float64 gradient), ``touched``
    (rows some position names) and ``bad_rows``.
    """
    uid, pid, nid = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (uid, pid, nid))
    B = uid.size
    assert 1 <= B < 2 ** 24 and pid.size == B and nid.size == B and 3 * B <= 15_000
    E = (rng.integers(-4, 5, size=(nu + ni, d)) / 4.0).astype(np.float32)
    coef = (rng.integers(0, 9, size=B) / 8.0).astype(np.float32)
    if sign is None:
        sign = int(rng.choice([-1, 1]))
    grad = np.array([sign * B * 2.0 ** m], dtype=np.float32)
    assert float(grad[0]) == sign * B * 2.0 ** m
    assert np.float32(-grad[0]) / np.float32(B) == -sign * 2.0 ** m
    fw = forward(E, nu, ni, uid, pid, nid)
    dE, mag = backward(E, nu, ni, uid, pid, nid, coef, grad[0])
    unit = 2.0 ** (m - 5)
    assert mag.max() / unit < 2 ** 24
    assert np.array_equal(np.round(dE / unit) * unit, dE)
    assert np.array_equal(dE.astype(np.float32).astype(np.float64), dE)
    assert d * 16 < 2 ** 24  # a dot's magnitudes sum to at most d: d·16 units
    assert np.array_equal(fw.s.astype(np.float32).astype(np.float64), fw.s)
    assert np.array_equal(np.round(fw.s * 16) / 16, fw.s)
    ru, rp, rn, _ = _rows(nu, ni, uid, pid, nid)
    touched = np.zeros(nu + ni, dtype=bool)
    touched[np.concatenate([ru, rp, rn])] = True
    return SimpleNamespace(E=E, nu=nu, ni=ni, d=d, B=B, uid=uid, pid=pid, nid=nid, coef=coef,
                           grad=grad, anc=fw.anc.astype(np.float32),
                           pos=fw.pos.astype(np.float32), s=fw.s, dE=dE.astype(np.float32),
                           touched=touched, bad_rows=fw.bad_rows)
