"""CPU: tests/_adam_ref.py, the float32 restatement that tests/test_gpu_adam_edges.py holds
hgd_adam_step's variant 0 to, checked here against the textbook Adam in float64 and against one
element worked out by hand. The 1e-6 below is a bound on the restatement, not on the kernel."""
import numpy as np
import pytest

from tests import _adam_ref as A

F32 = np.float32


def test_restatement_follows_float64_adam():
    """10 steps on 1,000 elements: p, m and v stay within 1e-6 relative of float64 Adam. Each
    element's gradients keep one sign, so that m is a sum without cancellation and a relative
    error of it means something."""
    rng = np.random.default_rng(7)
    n, steps = 1000, 10
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    sign = rng.choice([-1.0, 1.0], n)
    p = (rng.uniform(0.05, 0.2, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    m, v = np.zeros(n, F32), np.zeros(n, F32)
    p64, m64, v64 = p.astype(np.float64), np.zeros(n), np.zeros(n)
    table = A.scalar_rows([1], [(lr, betas, eps)], steps)
    worst = 0.0
    for k in range(steps):
        g = (10.0 ** rng.uniform(-3, 1, n) * sign).astype(F32)
        p, m, v = A.adam_step_v0(p, g, m, v, table[k, 0])
        p64, m64, v64 = A.adam_step_f64(p64, g.astype(np.float64), m64, v64, k + 1, lr, betas, eps)
        for a, b in ((p, p64), (m, m64), (v, v64)):
            assert a.dtype == np.float32
            worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b) / np.abs(b))))
    print(f"restatement vs float64 Adam, worst relative error over {steps} steps: {worst:.3g}")
    assert worst <= 1e-6


def test_one_element_by_hand():
    """p = 0.5, g = 2, m = v = 0 and scalars that are powers of two or 0.25 multiples:
    m = 0.5·(2 − 0) + 0 = 1;  v = 0·0.5 = 0, then 0.25·(2·2) + 0 = 1;
    d = sqrt(1) = 1, then 1/0.5 = 2, then 2 + 0.5 = 2.5;
    m/d = 1/2.5 rounds to 0x3ECCCCCD = 0.4000000059604645 (0.4 is not a float);
    −0.25·that = −0.10000000149011612 exactly; + 0.5 = 0.39999999850988388, which lies 7.5e-9
    below 0x3ECCCCCD and 2.2e-8 above 0x3ECCCCCC, so p = 0x3ECCCCCD."""
    s = np.array([0.5, 0.5, 0.25, 0.5, 0.5, -0.25], F32)
    one = lambda x: np.array([x], F32)
    p, m, v = A.adam_step_v0(one(0.5), one(2.0), one(0.0), one(0.0), s)
    assert p.view(np.uint32).tolist() == [0x3ECCCCCD]
    assert m.tolist() == [1.0] and v.tolist() == [1.0]


def test_scalar_rows_by_hand():
    """lr = 0.5, β = (0.5, 0.75), eps = 0.5. Step 1: bias corrections 0.5 and 0.25, all six
    exact. Step 2: 0.75 and 0.4375, whose root and quotient are rounded once from double."""
    rows = A.scalar_rows([1, 2], [(0.5, (0.5, 0.75), 0.5)] * 2, 1)
    assert rows.shape == (1, 2, 6) and rows.dtype == np.float32
    assert rows[0, 0].tolist() == [0.5, 0.75, 0.25, 0.5, 0.5, -1.0]
    assert rows[0, 1].tolist() == [0.5, 0.75, 0.25, float(F32(0.4375 ** 0.5)), 0.5,
                                   float(F32(-(0.5 / 0.75)))]
    # row k of tensor t is step first_steps[t] + k
    two = A.scalar_rows([1], [(0.5, (0.5, 0.75), 0.5)], 2)
    assert np.array_equal(two[1, 0], rows[0, 1])


def test_scalar_rows_are_reference_adams():
    """The same floats as optim.ReferenceAdam._build_table's expression, tensor by tensor."""
    import torch
    hyper, first = A.hypers(), A.first_steps()
    rows = []
    for k in range(A.TABLE_ROWS):
        for t0, (lr, (beta1, beta2), eps) in zip(first, hyper):
            t = t0 + k
            bc1 = 1 - beta1 ** t
            bc2 = 1 - beta2 ** t
            rows.append((1 - beta1, beta2, 1 - beta2, bc2 ** 0.5, eps, (lr / bc1) * -1))
    ref = torch.tensor(rows, dtype=torch.float64).to(torch.float32).reshape(
        A.TABLE_ROWS, len(hyper), 6).numpy()
    assert np.array_equal(ref.view(np.uint32), A.scalar_rows(first, hyper, A.TABLE_ROWS)
                          .view(np.uint32))
    # every tensor's row differs from its neighbours' and from the next step's
    tab = A.scalar_rows(first, hyper, A.TABLE_ROWS)
    for t in range(len(hyper) - 1):
        assert (tab[0, t] != tab[0, t + 1]).sum() >= 5
    assert all((tab[k] != tab[k + 1])[:, [3, 5]].all() for k in range(A.TABLE_ROWS - 1))


@pytest.mark.parametrize("bad", [1e-39, float("inf"), float("nan")])
def test_restatement_refuses_subnormal_and_non_finite(bad):
    s = np.array([0.1, 0.999, 0.001, 0.03, 1e-8, -1e-3], F32)
    one = lambda x: np.array([x], F32)
    with pytest.raises((AssertionError, FloatingPointError)):
        A.adam_step_v0(one(0.1), one(bad), one(0.0), one(0.0), s)
    with pytest.raises((AssertionError, FloatingPointError)):
        A.adam_step_v0(one(0.1), one(1e-30), one(0.0), one(0.0), s)  # g·g underflows


def test_problem_is_in_range():
    """The GPU test's data passes the restatement's range checks on every step."""
    params, grads, table = A.problem()
    assert [len(x) for x in params] == list(A.LENGTHS) and len(A.LENGTHS) == 16
    out = A.run(params, grads, table, range(A.STEPS))
    assert len(out) == A.STEPS
    for p, m, v in out:
        assert all(x.dtype == np.float32 for x in p + m + v)
