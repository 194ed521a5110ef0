"""GPU: functional.bpr_loss_rows' dispatch around the fused BPR kernels and bpr_index_errors.

* the per-device bad-index word: counted per batch row, kept by a non-resetting read, summed over
  calls, cleared by a resetting read, and still counted into by the replays of a captured step;
* negative but valid ids give what torch's own E[idx] gives (float64, the bounds of
  tests/test_gpu_hccf_layers.py's _check_bpr_rows);
* tables the kernels do not take (two tensors, a non-contiguous base, d = 10, d = 260, a
  misaligned base, an empty batch) go through the reference's torch ops, never the library;
* int32 ids and CPU ids are converted and take the fused path, bitwise as int64 device ids.
The kernels' own edges are tests/test_gpu_bpr_edges.py.
"""
import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from hypergraph_diffusion_for_recommendation_amd import functional as F

pytestmark = pytest.mark.gpu

NATIVE = ("hgd_bpr_forward", "hgd_bpr_backward")


def _table(dev, U, I, d, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (0.3 * torch.randn(U + I, d, device=dev, generator=g)).requires_grad_(True)


def _batch(dev, U, I, B, seed=1, lo=False):
    """Valid ids; with ``lo`` drawn from the whole torch range [-n, n)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randint(-n if lo else 0, n, (B,), device=dev, generator=g)
                 for n in (U, I, I))


def _count_calls(monkeypatch):
    """Lets the library's BPR entries through and counts their calls."""
    lib = nat.load()
    calls = {name: 0 for name in NATIVE}
    for name in NATIVE:
        real = getattr(lib, name)

        def counted(*args, _real=real, _name=name):
            calls[_name] += 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counted)
    return calls


def _forbid_native(monkeypatch):
    def no_call(*args):
        raise AssertionError("this table must not reach the library")
    lib = nat.load()
    for name in NATIVE:
        monkeypatch.setattr(lib, name, no_call)


def _run(ue, ie, ids, leaves, scale=2.5):
    loss, anc, pos = F.bpr_loss_rows(ue, ie, *ids)
    grads = torch.autograd.grad(scale * loss, leaves)
    return loss.detach(), anc.detach(), pos.detach(), grads


def _check_float64(got, leaves, split, ids, scale=2.5):
    """The bounds of _check_bpr_rows: loss 1e-6 relative, gathered rows bitwise, each gradient
    entry within 1e-5 · the sum of the magnitudes of its terms. ``split`` maps the float64
    leaves to (user table, item table); ids index those as torch does."""
    loss, anc, pos, grads = got
    uid, pid, nid = (t.cpu().long() for t in ids)
    B = uid.numel()
    l64 = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    u64, i64 = split(l64)
    a, p, n = u64[uid], i64[pid], i64[nid]
    ref = torch.mean(-torch.log(1e-5 + torch.sigmoid((a * p).sum(1) - (a * n).sum(1))))
    g64 = torch.autograd.grad(scale * ref, l64)
    ref = float(ref.detach())
    assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (float(loss), ref)
    assert torch.equal(anc.cpu().double(), a.detach()) and torch.equal(pos.cpu().double(),
                                                                       p.detach())
    # Σ|terms| of each gradient entry: the same chain on |·| (|coef| <= 1)
    m64 = [torch.zeros_like(t).requires_grad_(True) for t in l64]
    mu, mi = split(m64)
    w = scale / B
    U, I = u64.shape[0], i64.shape[0]
    a_, p_, n_ = a.detach().abs(), p.detach().abs(), n.detach().abs()
    surrogate = (mu[uid % U] * (w * (p_ + n_))).sum() + (mi[pid % I] * (w * a_)).sum() + \
        (mi[nid % I] * (w * a_)).sum()
    mags = torch.autograd.grad(surrogate, m64)
    for g, r, mag in zip(grads, g64, mags):
        err = (g.double().cpu() - r).abs()
        assert bool((err <= 1e-5 * mag + 1e-30).all()), float((err / (mag + 1e-30)).max())


def _one_block(leaves):
    return leaves[0][:U0], leaves[0][U0:]


def _two_tables(leaves):
    return leaves[0], leaves[1]


def _left_half(leaves):
    d = leaves[0].shape[1] // 2
    return leaves[0][:U0, :d], leaves[0][U0:, :d]


U0, I0 = 37, 53


# ---- bpr_index_errors -------------------------------------------------------------------------
@pytest.fixture
def fresh_word(monkeypatch):
    """A bad-index word of this test's own: the module keeps one per device for the process."""
    monkeypatch.setattr(F, "_BPR_BAD", {})


def _two_bad_rows(dev, B=64):
    uid, pid, nid = _batch(dev, U0, I0, B)
    uid[3], pid[3], nid[3] = U0, -I0 - 1, I0 + 5   # three bad ids: one row
    nid[40] = 2 ** 62
    uid[5], pid[6] = -U0, -1                       # valid
    return uid, pid, nid


def test_index_errors_count_rows_and_reset(dev, fresh_word):
    E = _table(dev, U0, I0, 16)
    ue, ie = torch.split(E, [U0, I0])
    assert F.bpr_index_errors(dev) == 0
    good = _batch(dev, U0, I0, 64, lo=True)
    F.bpr_loss_rows(ue, ie, *good)
    assert F.bpr_index_errors(dev) == 0
    bad = _two_bad_rows(dev)
    F.bpr_loss_rows(ue, ie, *bad)
    assert F.bpr_index_errors(dev, reset=False) == 2
    assert F.bpr_index_errors(dev, reset=False) == 2
    F.bpr_loss_rows(ue, ie, *bad)
    F.bpr_loss_rows(ue, ie, *good)
    assert F.bpr_index_errors(dev) == 4
    assert F.bpr_index_errors(dev) == 0
    F.bpr_loss_rows(ue, ie, *bad)
    assert F.bpr_index_errors(dev) == 2


def test_a_captured_step_keeps_counting(dev, fresh_word):
    """The forward alone (one branch, default queues), captured as tests/test_gpu_graph_step.py
    captures its steps: the word's address is fixed, so three replays of a batch with two bad
    rows add 6."""
    from hypergraph_diffusion_for_recommendation_amd.graphs import CapturedStep
    E = _table(dev, U0, I0, 32).detach()
    ue, ie = torch.split(E, [U0, I0])
    bad = _two_bad_rows(dev)

    def step(u, i, j):
        return F.bpr_loss_rows(ue, ie, u, i, j)[0]

    eager = step(*bad).clone()
    assert F.bpr_index_errors(dev) == 2
    cap = CapturedStep(step, bad)
    assert F.bpr_index_errors(dev, reset=False) == 0  # a capture runs nothing
    for _ in range(3):
        loss = cap(*bad)
    torch.cuda.synchronize()
    assert torch.equal(loss, eager)
    assert F.bpr_index_errors(dev) == 6
    cap(*_batch(dev, U0, I0, 64))
    assert F.bpr_index_errors(dev) == 0


# ---- negative but valid ids -------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 64, 256])
def test_negative_valid_ids_match_torch_indexing(dev, d, monkeypatch, fresh_word):
    calls = _count_calls(monkeypatch)
    E = _table(dev, U0, I0, d, seed=d)
    ue, ie = torch.split(E, [U0, I0])
    ids = list(_batch(dev, U0, I0, 257, seed=d, lo=True))
    ids[0][:3] = torch.tensor([-U0, -1, U0 - 1], device=dev)
    ids[1][:3] = torch.tensor([-1, -I0, I0 - 1], device=dev)
    ids[2][:3] = torch.tensor([-I0, -1, 0], device=dev)
    assert all(bool((t < 0).any()) for t in ids)
    got = _run(ue, ie, ids, [E])
    assert calls == {"hgd_bpr_forward": 1, "hgd_bpr_backward": 1}
    _check_float64(got, [E], _one_block, ids)
    assert F.bpr_index_errors(dev) == 0
    assert torch.equal(got[2][0], E.detach()[U0 + I0 - 1])  # pid = -1: the last item


# ---- fallbacks --------------------------------------------------------------------------------
def _misaligned(dev, N, d):
    """A root [N, d] tensor (no ._base) one float into its storage: data_ptr % 16 == 4."""
    flat = 0.3 * torch.randn(N * d + 4, device=dev)
    E = torch.empty(0, device=dev).set_(flat.untyped_storage(), 1, (N, d), (d, 1))
    assert E._base is None and E.data_ptr() % 16 == 4 and E.is_contiguous()
    return E.requires_grad_(True)


FALLBACKS = ["separate", "non_contiguous_base", "d10", "d260", "misaligned", "empty_batch"]


@pytest.mark.parametrize("kind", FALLBACKS)
def test_fallbacks_take_the_torch_path(dev, kind, monkeypatch):
    torch.manual_seed(5)
    d = {"d10": 10, "d260": 260}.get(kind, 16)
    ids = _batch(dev, U0, I0, 0 if kind == "empty_batch" else 130, lo=True)
    split = _one_block
    if kind == "separate":
        leaves = [_table(dev, U0, 0, d, seed=1), _table(dev, 0, I0, d, seed=2)]
        ue, ie = leaves
        split = _two_tables
    elif kind == "non_contiguous_base":
        leaves = [_table(dev, U0, I0, 2 * d)]
        base = leaves[0][:, :d]
        assert not base.is_contiguous()
        ue, ie = torch.split(base, [U0, I0])
        split = _left_half
    elif kind == "misaligned":
        leaves = [_misaligned(dev, U0 + I0, d)]
        ue, ie = torch.split(leaves[0], [U0, I0])
        assert F._table_of(ue, ie) is leaves[0]  # one block: only its address stops it
    else:
        leaves = [_table(dev, U0, I0, d)]
        ue, ie = torch.split(leaves[0], [U0, I0])
        assert F._table_of(ue, ie) is leaves[0]
    _forbid_native(monkeypatch)
    if kind == "empty_batch":
        loss, anc, pos = F.bpr_loss_rows(ue, ie, *ids)
        assert bool(torch.isnan(loss)) and anc.shape == pos.shape == (0, d)
        return
    _check_float64(_run(ue, ie, ids, leaves), leaves, split, ids)


def test_the_fallback_cases_differ_from_a_fused_one_only_as_stated(dev, monkeypatch):
    """The same one-block table at d = 16, aligned and with a batch, does reach the library: the
    fallbacks above are chosen by what each changes."""
    calls = _count_calls(monkeypatch)
    E = _table(dev, U0, I0, 16)
    ue, ie = torch.split(E, [U0, I0])
    ids = _batch(dev, U0, I0, 130, lo=True)
    _check_float64(_run(ue, ie, ids, [E]), [E], _one_block, ids)
    assert calls == {"hgd_bpr_forward": 1, "hgd_bpr_backward": 1}


# ---- id conversion ----------------------------------------------------------------------------
def test_int32_and_cpu_ids_take_the_fused_path(dev, monkeypatch):
    calls = _count_calls(monkeypatch)
    E = _table(dev, U0, I0, 64)
    ue, ie = torch.split(E, [U0, I0])
    ids = _batch(dev, U0, I0, 200, lo=True)
    base = _run(ue, ie, ids, [E])
    variants = {"int32": [t.int() for t in ids], "cpu": [t.cpu() for t in ids],
                "cpu int32": [t.cpu().int() for t in ids],
                "strided": [torch.stack([t, t + 1], 1)[:, 0] for t in ids]}
    assert not variants["strided"][0].is_contiguous()
    for k, (name, other) in enumerate(variants.items()):
        got = _run(ue, ie, other, [E])
        assert calls == {"hgd_bpr_forward": k + 2, "hgd_bpr_backward": k + 2}, name
        for a, b in zip(base[:3] + base[3], got[:3] + got[3]):
            assert torch.equal(a, b), name
