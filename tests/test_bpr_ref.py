"""CPU: tests/_bpr_ref64.py against torch's float64 autograd of the reference expression
(util/loss_torch.py:5-9 on the gathers of model/graph/HCCF.py:84-86), its index rule against
hand-written cases, and exact_case's promise at the largest shape tests/test_gpu_bpr_edges.py
uses."""
import numpy as np
import pytest
import torch

from tests import _bpr_ref64 as R

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _torch_reference(E, nu, uid, pid, nid, grad):
    E64 = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    a, p, n = E64[torch.as_tensor(uid)], E64[nu + torch.as_tensor(pid)], \
        E64[nu + torch.as_tensor(nid)]
    s = (a * p).sum(1) - (a * n).sum(1)
    s.retain_grad()
    loss = torch.mean(-torch.log(1e-5 + torch.sigmoid(s)))
    (grad * loss).backward()
    return a.detach().numpy(), p.detach().numpy(), s.detach().numpy(), float(loss.detach()), \
        s.grad.numpy(), E64.grad.numpy()


def _close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    scale = np.abs(ref).max() if ref.size else 0.0
    assert np.abs(got - ref).max() <= 1e-12 * scale, (what, float(np.abs(got - ref).max()), scale)


@pytest.mark.parametrize("nu,ni,d,B", [(5, 3, 8, 64), (40, 60, 12, 300), (7, 9, 60, 33)])
def test_forward_and_backward_are_torchs_float64_autograd(nu, ni, d, B):
    """Non-negative ids (torch indexes E[nu + pid], so a negative pid must be resolved first:
    the next test), many repeated rows and pid == nid in some rows."""
    rng = np.random.default_rng(nu * 1000 + d)
    E = rng.standard_normal((nu + ni, d)) * 0.5
    uid, pid, nid = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    nid[::5] = pid[::5]
    grad = 2.5
    a, p, s, loss, ds, dE = _torch_reference(E, nu, uid, pid, nid, grad)
    fw = R.forward(E, nu, ni, uid, pid, nid)
    assert np.array_equal(fw.anc, a) and np.array_equal(fw.pos, p)
    _close(fw.s, s, "s")
    assert (fw.s[::5] == 0).all()
    _close(fw.loss, loss, "loss")
    _close(fw.term.mean(), loss, "mean term")
    _close(-grad * fw.coef / B, ds, "coef")  # d(grad·loss)/ds_k = -grad·coef_k / B
    assert fw.bad_rows == 0
    got, mag = R.backward(E, nu, ni, uid, pid, nid, fw.coef, grad)
    _close(got, dE, "dE")
    assert (np.abs(got) <= mag * (1 + 1e-12)).all()
    untouched = np.ones(nu + ni, bool)
    untouched[np.concatenate([uid, nu + pid, nu + nid])] = False
    assert not got[untouched].any() and not mag[untouched].any()


def test_negative_ids_index_as_torch_does():
    """Each of the three id arrays indexes its own block: E[:nu][uid], E[nu:][pid], E[nu:][nid]
    with torch's negative ids, so pid = -1 is the last item, never a user."""
    rng = np.random.default_rng(3)
    nu, ni, d, B = 6, 4, 8, 50
    E = rng.standard_normal((nu + ni, d))
    uid, pid, nid = rng.integers(-nu, nu, B), rng.integers(-ni, ni, B), rng.integers(-ni, ni, B)
    pid[0], nid[1], uid[2] = -1, -ni, -nu
    E64 = torch.tensor(E, requires_grad=True)
    ue, ie = E64[:nu], E64[nu:]
    a, p, n = ue[torch.as_tensor(uid)], ie[torch.as_tensor(pid)], ie[torch.as_tensor(nid)]
    loss = torch.mean(-torch.log(1e-5 + torch.sigmoid((a * p).sum(1) - (a * n).sum(1))))
    (-1.5 * loss).backward()
    fw = R.forward(E, nu, ni, uid, pid, nid)
    assert np.array_equal(fw.anc, a.detach().numpy()) and np.array_equal(fw.pos, p.detach().numpy())
    assert np.array_equal(fw.pos[0], E[nu + ni - 1]) and fw.bad_rows == 0
    _close(fw.loss, float(loss.detach()), "loss")
    _close(R.backward(E, nu, ni, uid, pid, nid, fw.coef, -1.5)[0], E64.grad.numpy(), "dE")


def test_saturated_scores_stay_finite():
    E = np.zeros((2, 4))
    E[0, 0] = 1.0
    for s, term, coef in ((200.0, -np.log(1 + 1e-5), 0.0), (-200.0, -np.log(1e-5), 0.0),
                          (0.0, -np.log(0.5 + 1e-5), 0.25 / (0.5 + 1e-5))):
        E[1, 0] = s
        T = np.vstack([E, np.zeros((1, 4))])  # user 0, items: row 1 (positive), row 2 (zero)
        fw = R.forward(T, 1, 2, [0], [0], [1])
        assert fw.s[0] == s and np.isfinite([fw.term[0], fw.coef[0], fw.loss]).all()
        assert abs(fw.term[0] - term) <= 1e-15 + 1e-12 * abs(term)
        assert abs(fw.coef[0] - coef) <= 1e-15 + 1e-12 * abs(coef)


def test_resolve():
    n = 7
    ids = [0, 3, n - 1, -1, -n, n, -n - 1, 2 ** 62, -2 ** 62, I64_MAX, I64_MIN, 2 ** 62 + 1]
    rows, bad = R.resolve(np.array(ids, dtype=np.int64), n)
    assert rows.tolist() == [0, 3, 6, 6, 0, 6, 0, 6, 0, 6, 0, 6]
    assert bad.tolist() == [False] * 5 + [True] * 7
    rows, bad = R.resolve(np.array([0, -1, 1, -2, I64_MAX, I64_MIN], dtype=np.int64), 1)
    assert rows.tolist() == [0] * 6 and bad.tolist() == [False, False, True, True, True, True]
    rows, bad = R.resolve(np.zeros(0, np.int64), 3)
    assert rows.size == 0 and bad.size == 0 and rows.dtype == np.int64


def test_bad_rows_counts_rows_not_ids():
    E = np.ones((5, 4))
    fw = R.forward(E, 2, 3, [0, 2, 0, -3, 1], [0, 3, 3, 0, -3], [0, -4, 0, 0, 2])
    assert fw.bad_rows == 3  # row 1 holds three bad ids, rows 2 and 3 one each
    assert np.array_equal(fw.anc[1], E[1]) and np.array_equal(fw.pos[2], E[4])


def test_exact_case_keeps_its_promise_at_the_largest_shape():
    """B = 4,110 at d = 256 (12,330 positions), a row hit by a third of them, and a larger power
    of two than the device tests scale grad by."""
    rng = np.random.default_rng(11)
    nu, ni, d, B = 30, 40, 256, 4110
    uid, pid, nid = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    pid[: B // 2] = 5
    nid[B // 2:] = 5
    c = R.exact_case(rng, nu, ni, d, uid, pid, nid, m=3)
    assert c.dE.dtype == np.float32 and c.dE.shape == (nu + ni, d) and c.touched.all()
    ref, _ = R.backward(c.E, nu, ni, uid, pid, nid, c.coef, c.grad[0])
    assert np.array_equal(c.dE.astype(np.float64), ref) and np.abs(ref).max() > 100
    # float32 sums of the same terms in two unrelated orders give that very result
    t = (-c.grad[0] / np.float32(B)) * c.coef
    for order in (np.arange(B), rng.permutation(B)):
        acc = np.zeros(d, np.float32)
        for k in order[pid[order] == 5]:
            acc += t[k] * c.E[uid[k]]
        for k in order[nid[order] == 5]:
            acc += -t[k] * c.E[uid[k]]
        assert acc.dtype == np.float32 and np.array_equal(acc, c.dE[nu + 5])
    assert set(np.unique(c.E * 4)) <= set(range(-4, 5)) and set(np.unique(c.coef * 8)) <= set(range(9))
