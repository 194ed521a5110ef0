"""hgd_row_epilogue_backward_dt through the C ABI: the fused row epilogue's backward with dZ stored
in bfloat16.

Statements:
  * forwarding: with HGD_DT_F32 it is hgd_row_epilogue_backward, bit for bit (dZ, dγ, dβ);
  * rounding: with HGD_DT_BF16, dZ is bitwise torch's bfloat16 cast of the fp32 entry point's dZ on
    the same inputs — the arithmetic is the fp32 one and the store rounds to nearest even once —
    and dγ / dβ, summed from the unrounded values, are bitwise the fp32 entry point's; a second
    run is bitwise the first.
The fp32 entry point is the reference throughout (tests/test_gpu_fused.py holds it to the float64
oracle), always on the same kernel form as the call under test: the LayerNorm sums are a butterfly
over the lane group, so a call that the alignment sends to one column per lane is compared with
an fp32 call sent there too (its dZ one float off the 16-byte grid).

Shapes: every lane-group size of the four-column path (d = 8 … 256: 2 … 64 lanes), d = 5 and 20,
each with LayerNorm alone, LeakyReLU(0.2) with and without LayerNorm and ReLU without, with and
without γ; 1, 7 and 500 rows; 4,099 rows at d = 256 (more than 1,024 blocks × 4 rows: the grid
stride with a ragged last sweep); d = 320 without LayerNorm (two column passes, the second 64
wide); a padded ldz whose poison must survive; a dZ one bf16 element off the 8-byte grid; and
dY with ±0, a denormal, ±inf and a NaN.
"""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
WIDTHS = [8, 16, 64, 128, 256]
UNALIGNED = [5, 20]
OUT_SCALE = 0.7
# act, slope, LayerNorm
CONFIGS = [(None, 0.0, True), ("leaky_relu", 0.2, True), ("leaky_relu", 0.2, False),
           ("relu", 0.0, False)]
POISON = 9.0


def _inputs(n, d, act, ln, with_gamma, seed, dev):
    """dY, act_out (a = act(z) of a random z), the LayerNorm statistics of a, γ."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, d)).astype(np.float32)
    a = {None: z, "leaky_relu": np.where(z > 0, z, np.float32(0.2) * z),
         "relu": np.maximum(z, 0)}[act].astype(np.float32)
    o = dict(n=n, d=d, act=act, ln=ln)
    o["dY"] = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    o["A"] = torch.from_numpy(a).to(dev) if ln or act is not None else None
    o["stats"] = o["gamma"] = None
    if ln:
        mu = a.mean(-1, dtype=np.float64)
        rstd = 1.0 / np.sqrt(a.var(-1, dtype=np.float64) + 1e-5)
        o["stats"] = torch.from_numpy(np.stack([mu, rstd], 1).astype(np.float32)).to(dev)
        if with_gamma:
            o["gamma"] = torch.from_numpy((rng.random(d) + 0.5).astype(np.float32)).to(dev)
    return o


def _call(o, slope, dtype, ldz=None, offset=0, entry="dt"):
    """One call; dZ is a [n, d] view at element ``offset`` of a poisoned buffer of leading
    dimension ``ldz``. ``entry``: "dt" (with the code of ``dtype``) or "fp32" (the fp32 entry
    point; ``dtype`` is float32). Returns (dZ view, whole buffer, dγ, dβ)."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    n, d, ln = o["n"], o["d"], o["ln"]
    dev = o["dY"].device
    ldz = d if ldz is None else ldz
    buf = torch.full((n * ldz + offset,), POISON, dtype=dtype, device=dev)
    dZ = buf[offset:].view(n, ldz)[:, :d]
    assert dZ.data_ptr() == buf.data_ptr() + offset * buf.element_size()
    dg = torch.full((d,), POISON, device=dev) if ln else None
    db = torch.full((d,), POISON, device=dev) if ln else None
    wsb = lib.hgd_row_epilogue_backward_workspace_size(n, d) if ln else 0
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev) if wsb else None
    epi = {None: nat.EPI_NONE, "leaky_relu": nat.EPI_LEAKY_RELU, "relu": nat.EPI_RELU}[o["act"]]
    A = o["A"]
    head = [o["dY"].data_ptr(), o["dY"].stride(0), nat.ptr(A), 0 if A is None else A.stride(0),
            nat.ptr(o["stats"]), nat.ptr(o["gamma"]), n, d, epi, slope, int(ln), OUT_SCALE,
            dZ.data_ptr()]
    tail = [ldz, nat.ptr(dg), nat.ptr(db), nat.ptr(ws), wsb, nat.stream_handle(dev)]
    if entry == "fp32":
        assert dtype == F32
        nat.check(lib.hgd_row_epilogue_backward(*head, *tail), "hgd_row_epilogue_backward")
    else:
        code = {F32: nat.DT_F32, BF16: nat.DT_BF16}[dtype]
        nat.check(lib.hgd_row_epilogue_backward_dt(*head, code, *tail),
                  "hgd_row_epilogue_backward_dt")
    return dZ, buf, dg, db


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return a is b is None or torch.equal(_bits(a), _bits(b))


def _check(o, slope, ldz=None, offset16=0, offset32=0):
    """The three statements for one input set. ``offset16`` / ``offset32``: where the bf16 call's
    and the fp32 reference's dZ start in their buffers."""
    n, d = o["n"], o["d"]
    ref, rbuf, rg, rb = _call(o, slope, F32, ldz, offset32, entry="fp32")
    assert not bool((ref == POISON).any())
    fwd, fbuf, fg, fb = _call(o, slope, F32, ldz, offset32)
    assert _same(fbuf, rbuf) and _same(fg, rg) and _same(fb, rb)
    got, gbuf, gg, gb = _call(o, slope, BF16, ldz, offset16)
    assert got.dtype == BF16
    assert _same(got, ref.bfloat16()), f"dZ is not the rounded fp32 dZ (n={n}, d={d})"
    assert _same(gg, rg) and _same(gb, rb)
    again, abuf, ag, ab = _call(o, slope, BF16, ldz, offset16)
    assert _same(abuf, gbuf) and _same(ag, gg) and _same(ab, gb)
    # nothing outside the [n, d] view is written
    w = d if ldz is None else ldz
    if offset16:
        assert bool((gbuf[:offset16] == POISON).all())
    if w > d:
        assert bool((gbuf[offset16:].view(n, w)[:, d:] == POISON).all())
        assert bool((rbuf[offset32:].view(n, w)[:, d:] == POISON).all())
    return got


# ---- forwarding, rounding, determinism over the kernel forms ------------------------------------
@gpu
@pytest.mark.parametrize("d", WIDTHS + UNALIGNED)
def test_bf16_dz_is_the_rounded_fp32_dz(dev, d):
    for i, (act, slope, ln) in enumerate(CONFIGS):
        for with_gamma in ((False, True) if ln else (False,)):
            for n in (1, 7, 500):
                o = _inputs(n, d, act, ln, with_gamma, 1000 * d + 10 * i + n, dev)
                got = _check(o, slope)
                assert bool(got.float().abs().sum() > 0)


@gpu
def test_grid_stride_with_a_ragged_last_sweep(dev):
    """4,099 rows at d = 256: 4 rows per block, 1,024 blocks — every block walks two rows, three
    of them a third one."""
    for with_gamma in (False, True):
        _check(_inputs(4099, 256, "leaky_relu", True, with_gamma, 5, dev), 0.2)


@gpu
def test_wide_row_two_column_passes(dev):
    """d = 320 without LayerNorm: a 256-column pass of 64 lanes, then one over the last 64
    columns in which 48 lanes of every group store nothing."""
    for act, slope in (("leaky_relu", 0.2), ("relu", 0.0)):
        for n in (7, 500):
            _check(_inputs(n, 320, act, False, False, 6 + n, dev), slope)
            _check(_inputs(n, 320, act, False, False, 7 + n, dev), slope, ldz=324)


@gpu
@pytest.mark.parametrize("d", [8, 64, 256, 20])
def test_padded_ldz_keeps_its_poison(dev, d):
    """ldz = d + 4 stays on the vector path, d + 3 leaves it (for both element types, so the
    reference is on the same form; LayerNorm there up to d = 64)."""
    for act, slope, ln in CONFIGS:
        _check(_inputs(37, d, act, ln, True, 8 + d, dev), slope, ldz=d + 4)
        if not ln or d <= 64:
            _check(_inputs(37, d, act, ln, True, 9 + d, dev), slope, ldz=d + 3)


@gpu
@pytest.mark.parametrize("d,ln", [(64, True), (16, True), (128, False), (320, False)])
def test_dz_one_element_off_the_grid_takes_the_one_column_path(dev, d, ln):
    """A dZ pointer one bf16 element past an aligned one (2 bytes off the 8-byte grid): one column
    per lane, the same rounding. The reference's dZ is one float off, so it is on that form too."""
    for n in (7, 500):
        o = _inputs(n, d, "leaky_relu", ln, True, 11 + d + n, dev)
        got = _check(o, 0.2, offset16=1, offset32=1)
        if not ln:
            # no sum over the lanes: the form does not show in dZ, so the aligned call agrees
            assert _same(got, _check(o, 0.2))


# ---- special values ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d,ln", [(64, False), (5, False), (64, True)])
def test_special_values(dev, d, ln):
    """±0, a denormal, ±inf and a NaN in dY: dZ matches torch's cast of the fp32 dZ bit for bit,
    NaN payloads aside (their positions are compared). With LayerNorm a row that holds an inf or
    a NaN is NaN throughout, as in fp32."""
    n = 9
    o = _inputs(n, d, "leaky_relu", ln, True, 13 + d, dev)
    special = [0.0, -0.0, 1e-40, -1e-40, float("inf"), float("-inf"), float("nan"),
               2.0 ** -126, 3.4028234e38]  # the smallest normal and the largest finite float32
    dY = o["dY"].clone()
    for k, v in enumerate(special):
        dY[k, (3 * k) % d] = v          # one per row, on either branch of the activation
        dY[(k + 1) % n, (3 * k + 1) % d] = v
    o["dY"] = dY
    ref, _, rg, rb = _call(o, 0.2, F32, entry="fp32")
    got, _, gg, gb = _call(o, 0.2, BF16)
    want = ref.bfloat16()
    nan = torch.isnan(ref)
    assert bool(nan.any())
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])
    if not ln:  # every special value reaches dZ on its own
        assert bool(torch.isinf(ref).any()) and bool((ref == 0).any())
        assert int(nan.sum()) == 2
    if ln:
        for a, b in ((gg, rg), (gb, rb)):
            assert torch.equal(torch.isnan(a), torch.isnan(b))
            ok = ~torch.isnan(a)
            assert torch.equal(_bits(a)[ok], _bits(b)[ok])
    again, _, _, _ = _call(o, 0.2, BF16)
    assert torch.equal(_bits(again)[~nan], _bits(got)[~nan])
