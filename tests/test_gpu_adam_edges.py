"""GPU: hgd_adam_step called through the C ABI at the edges of csrc/adam.hip.

The reference is tests/_adam_ref.py: a float32 numpy restatement of variant 0 (checked on the CPU
by tests/test_adam_ref.py), compared bit for bit. Every array of a call (the four per tensor, the
scalar table, the row index) is carved out of one guarded device buffer (tests/_arena.py); after
every launch the guards, the gradients and the table must be bytewise unchanged.

What the 16 lengths reach in k_adam, which the model-level tests never do:
  * the ``block0[t + 1]`` walk over a zero-length tensor first, in the middle and last, and over
    the most tensors a launch takes;
  * ``e + 4 <= n`` false inside a chunk (1, 3, 5, 255, 1023, 1025, ... : the float4 path's partial
    last vector) and tensors ending within one element of a 1024-element unroll step and of one
    and two 4096-element chunks;
  * ``L.vec[t] == 0``: the element-wise path, chosen when any one of the four arrays is off a
    16-byte boundary;
  * ``table[(row·count + t)·6 ...]`` with 16 different scalar rows per step and 4 steps.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from tests import _adam_ref as A
from tests._arena import Arena, bits

pytestmark = pytest.mark.gpu

COUNT = len(A.LENGTHS)
# byte offsets from a 16-byte boundary of (param, grad, exp_avg, exp_avg_sq)
LAYOUTS = {"aligned": (0, 0, 0, 0), "all_off": (4, 4, 4, 4), "grad_off": (0, 4, 0, 0),
           "sq_off": (0, 0, 0, 4)}


@functools.lru_cache(maxsize=None)
def _problem():
    params, grads, table = A.problem()
    for x in params + [g for step in grads for g in step] + [table]:
        x.flags.writeable = False
    return params, grads, table


@functools.lru_cache(maxsize=None)
def _reference(first_row, steps):
    params, grads, table = _problem()
    return A.run(params, grads, table, range(first_row, first_row + steps))


def _arena(dev, layout, first_row=0):
    params, grads, table = _problem()
    off = LAYOUTS[layout]
    ar = Arena()
    for t in range(COUNT):
        ar.add(f"p{t}", params[t], off[0], out=True)
        ar.add(f"g{t}", grads[0][t], off[1])
        ar.add(f"m{t}", np.zeros_like(params[t]), off[2], out=True)
        ar.add(f"v{t}", np.zeros_like(params[t]), off[3], out=True)
    ar.add("table", table)
    ar.add("row", np.array([first_row], np.int32), out=True)
    ar.add("idle", np.array([2], np.int32))  # a word no call is given: it must keep its 2
    ar.upload(dev)
    for t in range(COUNT):
        for k, name in enumerate("pgmv"):
            assert ar.ptr(f"{name}{t}") % 16 == off[k]
    return ar


def _tensors(ar):
    arr = (nat.AdamTensor * COUNT)()
    for t, n in enumerate(A.LENGTHS):
        arr[t].param, arr[t].grad = ar.ptr(f"p{t}"), ar.ptr(f"g{t}")
        arr[t].exp_avg, arr[t].exp_avg_sq = ar.ptr(f"m{t}"), ar.ptr(f"v{t}")
        arr[t].n = n
    return arr


def _step(dev, ar, arr, variant, with_row=True, count=COUNT):
    st = nat.load().hgd_adam_step(ctypes.cast(arr, ctypes.c_void_p), count, ar.ptr("table"),
                                  ar.ptr("row") if with_row else None, variant,
                                  nat.stream_handle(dev))
    nat.check(st, "hgd_adam_step")


def _run(dev, layout, variant, steps=A.STEPS, first_row=0, with_row=True):
    """The (p, m, v) lists after each of ``steps`` launches; guards, gradients, table and the
    idle word checked after each, and the row index that it advanced by one (or, with a NULL
    step_row, that nothing moved it)."""
    _, grads, _ = _problem()
    ar = _arena(dev, layout, first_row)
    arr = _tensors(ar)
    states = []
    for k in range(steps):
        for t in range(COUNT):
            ar.write(f"g{t}", grads[k][t])
        _step(dev, ar, arr, variant, with_row)
        outs = ar.check((layout, variant, k))
        assert outs["row"].tolist() == [first_row + k + 1 if with_row else first_row]
        states.append(tuple([outs[f"{name}{t}"] for t in range(COUNT)] for name in "pmv"))
    return states


def _assert_bitwise(got, ref, what, rows=None):
    _, _, table = _problem()
    for k, (gs, rs) in enumerate(zip(got, ref)):
        for name, g_list, r_list in zip(("param", "exp_avg", "exp_avg_sq"), gs, rs):
            for t, (g, r) in enumerate(zip(g_list, r_list)):
                assert g.shape == r.shape
                diff = np.flatnonzero(bits(g) != bits(r))
                if diff.size:
                    e = int(diff[0])
                    scal = None if rows is None else table[rows[k], t].tolist()
                    raise AssertionError(
                        f"{what}: launch {k}, tensor {t} (n = {A.LENGTHS[t]}), {name}[{e}] = "
                        f"{g[e]!r} ({bits(g)[e]:#010x}), expected {r[e]!r} ({bits(r)[e]:#010x}); "
                        f"{diff.size} elements differ; scalars {scal}")


# ---- a, b: lengths and bases, against the restatement -----------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_variant0_is_the_restatement(dev, layout):
    """Three steps (table rows 0, 1, 2, the kernel advancing the row itself), 16 tensors, each
    with its own scalars: param, exp_avg and exp_avg_sq bitwise the numpy restatement after every
    step, at 16-byte aligned bases (the float4 path with its partial last vector) and with all,
    only grad or only exp_avg_sq one float past a boundary (the element-wise path)."""
    got = _run(dev, layout, 0)
    _assert_bitwise(got, _reference(0, A.STEPS), layout, rows=range(A.STEPS))


def test_neighbouring_scalars_would_show(dev):
    """The check above can see a wrong table index: the restatement run with tensor t + 1's
    scalars, or with the next row, differs from the device's result in every non-empty tensor."""
    params, grads, table = _problem()
    got = _run(dev, "aligned", 0, steps=1)[0]
    shifted = A.run(params, grads, np.roll(table, -1, axis=1), [0])[0]
    next_row = A.run(params, grads, table, [1])[0]
    for wrong in (shifted, next_row):
        for t, n in enumerate(A.LENGTHS):
            if n:
                assert (bits(got[0][t]) != bits(wrong[0][t])).any(), t


# ---- c: both paths run the same adam_one, in every variant ------------------------------------
@pytest.mark.parametrize("variant", range(32))
def test_aligned_and_unaligned_agree_in_every_variant(dev, variant):
    a = _run(dev, "aligned", variant)
    b = _run(dev, "all_off", variant)
    _assert_bitwise(b, a, f"variant {variant}, unaligned against aligned")


def test_the_variant_reaches_both_paths(dev):
    """The agreement above is not that of a kernel which ignores ``variant``: fusing any one of
    the three multiply-adds changes bits somewhere in 37,000 elements, on either path."""
    for layout in ("aligned", "all_off"):
        base = _run(dev, layout, 0, steps=2)[1]  # the moments are zero before step 1
        for variant in (1, 2, 4):
            other = _run(dev, layout, variant, steps=2)[1]
            assert any((bits(a) != bits(b)).any() for x, y in zip(base, other)
                       for a, b in zip(x, y)), (layout, variant)


# ---- d: the calibrated variant at these lengths -----------------------------------------------
def test_calibrated_variant_is_torch_adam_at_these_lengths(dev):
    from hypergraph_diffusion_for_recommendation_amd.optim import ReferenceAdam
    params, grads, _ = _problem()
    keep = [t for t, n in enumerate(A.LENGTHS) if n]
    p0 = [torch.tensor(params[t], device=dev) for t in keep]
    rng = np.random.default_rng(5)
    steps = 5
    gr = [[torch.tensor((10.0 ** rng.uniform(-3, 1, len(p)) * rng.choice([-1.0, 1.0], len(p)))
                        .astype(np.float32), device=dev) for p in p0] for _ in range(steps)]

    def groups(ps):  # two groups with their own lr and betas
        return [dict(params=ps[0::2], lr=1e-3), dict(params=ps[1::2], lr=3e-3, betas=(0.8, 0.99))]

    ref = [p.clone().requires_grad_(True) for p in p0]
    mine = [p.clone().requires_grad_(True) for p in p0]
    topt = torch.optim.Adam(groups(ref), foreach=True)
    ropt = ReferenceAdam(groups(mine))
    for k in range(steps):
        for a, b, g in zip(ref, mine, gr[k]):
            a.grad, b.grad = g.clone(), g.clone()
        topt.step()
        ropt.step()
        for t, a, b in zip(keep, ref, mine):
            assert torch.equal(a.detach(), b.detach()), (k, A.LENGTHS[t])
    for t, a, b in zip(keep, ref, mine):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(topt.state[a][key], ropt.state[b][key]), (key, A.LENGTHS[t])


# ---- e: the row index -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["aligned", "all_off"])
def test_device_row_index_selects_the_row(dev, layout):
    """step_row holds 2 in a table of 4 rows: row 2 is read, and step_row is 3 afterwards."""
    got = _run(dev, layout, 0, steps=1, first_row=2)
    _assert_bitwise(got, _reference(2, 1), "row 2", rows=[2])
    assert any((bits(a) != bits(b)).any()
               for a, b in zip(_reference(2, 1)[0][0], _reference(0, 1)[0][0]))


@pytest.mark.parametrize("layout", ["aligned", "all_off"])
def test_null_row_index_reads_row_0_and_advances_nothing(dev, layout):
    """A NULL step_row: row 0, and no advance kernel runs. The arena's own row word (2, not
    passed) and the idle word (2) both still hold 2, checked in _run."""
    got = _run(dev, layout, 0, steps=1, first_row=2, with_row=False)
    _assert_bitwise(got, _reference(0, 1), "NULL step_row", rows=[0])


# ---- f: rejections leave every buffer alone ---------------------------------------------------
def test_rejections_touch_nothing(dev):
    """The refusals of tests/test_adam_rejections.py with real buffers behind the pointers: a
    non-zero status, a message, and every byte of the buffer as it was."""
    lib = nat.load()
    ar = _arena(dev, "aligned")
    st = nat.stream_handle(dev)
    table, row = ar.ptr("table"), ar.ptr("row")

    def call(arr, count, scalars=table, step_row=row, variant=0):
        return lib.hgd_adam_step(ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None,
                                 count, scalars, step_row, variant, st)

    def edited(t, **fields):
        arr = _tensors(ar)
        for k, v in fields.items():
            setattr(arr[t], k, v)
        return arr

    big = (nat.AdamTensor * 17)()
    for t in range(17):
        big[t].n = 0
    bad = [call(_tensors(ar), 0), call(big, 17), call(None, COUNT),
           call(_tensors(ar), COUNT, variant=-1), call(_tensors(ar), COUNT, variant=32),
           call(_tensors(ar), COUNT, scalars=None), call(edited(5, n=-1), COUNT)]
    bad += [call(edited(t, **{f: None}), COUNT)
            for t in (1, 14) for f in ("param", "grad", "exp_avg", "exp_avg_sq")]
    for status in bad:
        assert status != 0
    # each refusal leaves its message
    assert call(edited(14, grad=None), COUNT) != 0
    assert lib.hgd_get_last_error_string().decode() == \
        "hgd_adam_step: tensor 14 has a null pointer"
    outs = ar.check("after the refusals")
    params, _, _ = _problem()
    assert outs["row"].tolist() == [0]
    for t in range(COUNT):
        assert np.array_equal(bits(outs[f"p{t}"]), bits(params[t]))
        assert not outs[f"m{t}"].any() and not outs[f"v{t}"].any()


def test_null_arrays_of_an_empty_tensor_are_accepted(dev):
    """n == 0 with four NULL pointers, first, in the middle and last: the launch is the same."""
    _, grads, _ = _problem()
    ar = _arena(dev, "aligned")
    arr = _tensors(ar)
    for t, n in enumerate(A.LENGTHS):
        if n == 0:
            arr[t].param = arr[t].grad = arr[t].exp_avg = arr[t].exp_avg_sq = None
    _step(dev, ar, arr, 0)
    outs = ar.check("NULL empty tensors")
    assert outs["row"].tolist() == [1]
    got = [tuple([outs[f"{name}{t}"] for t in range(COUNT)] for name in "pmv")]
    _assert_bitwise(got, _reference(0, 1), "NULL empty tensors", rows=[0])
    # a launch of empty tensors only runs the advance alone
    only = (nat.AdamTensor * 2)()
    _step(dev, ar, only, 0, count=2)
    assert ar.check("empty launch")["row"].tolist() == [2]
