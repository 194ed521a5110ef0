"""A numpy restatement of one hgd_adam_step element, variant 0, and of the scalar rows it reads.

Variant 0 of csrc/adam.hip fuses nothing and uses the correctly rounded square root and division,
so every ``*``, ``+``, ``-``, ``/`` and ``sqrt`` below is one IEEE float32 operation, rounded on
its own, in the order of the kernel's header:

    m = s0*(g - m) + m
    v = v*s1 ; v = s2*(g*g) + v
    d = sqrt(v) ; d = d/s3 ; d = d + s4
    p = s5*(m/d) + p

numpy's float32 arithmetic rounds each operation the same way, so this is a bit-exact model of
the kernel, independent of torch and of optim.calibrated_variant. Every input and intermediate is
required to be finite and either zero or of normal magnitude, so no flush-to-zero mode of either
side can matter; a product may be zero only where a factor is.

``scalar_rows`` restates optim.ReferenceAdam._build_table: Python doubles, rounded once to float32.
"""
import numpy as np

F32 = np.float32
_TINY = np.finfo(np.float32).tiny


def _normal(x, what):
    x = np.asarray(x)
    assert x.dtype == np.float32, (what, x.dtype)
    assert np.isfinite(x).all(), f"{what}: non-finite"
    assert ((x == 0) | (np.abs(x) >= _TINY)).all(), f"{what}: subnormal"
    return x


def _mul(a, b, what):
    r = _normal(a * b, what)
    assert ((r != 0) | (np.asarray(a) == 0) | (np.asarray(b) == 0)).all(), f"{what}: underflow"
    return r


def adam_step_v0(p, g, m, v, s):
    """One step of every element: float32 arrays p, g, m, v and the six float32 scalars s.
    Returns the new (p, m, v); the arguments are left unchanged."""
    p, g, m, v = (_normal(x, n) for x, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")))
    s = _normal(np.asarray(s), "scalars")
    assert s.shape == (6,)
    with np.errstate(all="raise", under="ignore"):  # an underflow is caught by _normal / _mul
        m = _normal(_mul(s[0], _normal(g - m, "g-m"), "s0*(g-m)") + m, "m")
        v = _mul(v, s[1], "v*s1")
        v = _normal(_mul(s[2], _mul(g, g, "g*g"), "s2*(g*g)") + v, "v")
        d = _normal(np.sqrt(v), "sqrt(v)")
        d = _normal(d / s[3], "d/s3")
        d = _normal(d + s[4], "d+s4")
        assert (d > 0).all(), "m/d: zero denominator"
        q = _normal(m / d, "m/d")
        assert ((q != 0) | (m == 0)).all(), "m/d: underflow"
        p = _normal(_mul(s[5], q, "s5*(m/d)") + p, "p")
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def scalar_row(step, lr, betas, eps):
    """The six doubles of one (step, tensor), as ReferenceAdam._build_table computes them."""
    beta1, beta2 = betas
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return (1 - beta1, beta2, 1 - beta2, bc2 ** 0.5, eps, (lr / bc1) * -1)


def scalar_rows(first_steps, hypers, n_rows):
    """float32 [n_rows, count, 6]: row k holds tensor t's scalars at step first_steps[t] + k.
    hypers[t] = (lr, (beta1, beta2), eps)."""
    assert len(first_steps) == len(hypers)
    rows = [scalar_row(t0 + k, *h) for k in range(n_rows) for t0, h in zip(first_steps, hypers)]
    return np.array(rows, dtype=np.float64).astype(np.float32).reshape(n_rows, len(hypers), 6)


def adam_step_f64(p, g, m, v, step, lr, betas, eps):
    """The textbook Adam (Kingma & Ba, algorithm 1, eps outside the bias-corrected root) in
    float64."""
    beta1, beta2 = betas
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    m_hat = m / (1 - beta1 ** step)
    v_hat = v / (1 - beta2 ** step)
    return p - lr * m_hat / (np.sqrt(v_hat) + eps), m, v


# ---- the data of tests/test_gpu_adam_edges.py, built once ---------------------------------------
# One launch of 16 tensors (the most a launch takes): a zero-length tensor first, in the middle and
# last; lengths below one float4, a float4 and one more, and within one of a 1024-element unroll
# step and of one and two 4096-element chunks.
LENGTHS = (0, 1, 3, 4, 5, 255, 1023, 0, 1024, 1025, 4095, 4096, 4097, 8191, 8195, 0)
STEPS = 3
TABLE_ROWS = 4


def hypers():
    """Every tensor its own lr, betas and eps (so another tensor's scalars give other bits)."""
    return [(1e-3 * (1 + 0.25 * t), (0.9 - 0.01 * t, 0.999 - 0.002 * t), 1e-8 * (1 + t))
            for t in range(len(LENGTHS))]


def first_steps():
    """Every tensor its own step count at row 0 (so another row gives other bits)."""
    return [1 + 2 * t for t in range(len(LENGTHS))]


def problem(seed=20):
    """(params, grads[step], table): |p| about 0.1, |g| log-uniform in [1e-3, 10] of either sign,
    the moments zero as a fresh optimizer's."""
    rng = np.random.default_rng(seed)
    params = [(rng.uniform(0.05, 0.2, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
              for n in LENGTHS]
    grads = [[(10.0 ** rng.uniform(-3, 1, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
              for n in LENGTHS] for _ in range(TABLE_ROWS)]
    table = scalar_rows(first_steps(), hypers(), TABLE_ROWS)
    return params, grads, table


def run(params, grads, table, rows):
    """State after each launch, launch k reading table row rows[k] and grads[k]:
    a list of (p, m, v), each a list over the tensors."""
    p = [x.copy() for x in params]
    m = [np.zeros_like(x) for x in params]
    v = [np.zeros_like(x) for x in params]
    out = []
    for k, row in enumerate(rows):
        for t in range(len(p)):
            p[t], m[t], v[t] = adam_step_v0(p[t], grads[k][t], m[t], v[t], table[row, t])
        out.append(([x.copy() for x in p], [x.copy() for x in m], [x.copy() for x in v]))
    return out
