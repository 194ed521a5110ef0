"""hgd_gemm_tn at every kernel form against float64 (tests/_gemm_ref64.py): the f32-MFMA split-K
kernel (HGD_TUNE_X3_SPLITK = 0, HGD_TUNE_GEMM_EXACT = 1), the one-wave-per-tile split-bf16 kernel
(HGD_TUNE_X3_SPLITK = 1), the producer-wave kernel in its barrier and queue forms (by shape;
HGD_TUNE_X3P_QUEUE = 1), each under the default slice sizing and HGD_TUNE_SPLITK_ROWS = 64, 192,
4096 — shapes up to 272 columns, ragged slices, leading dimensions above the width, every option,
groups with empty and very unequal members, the workspace size and its guard, determinism."""
import numpy as np
import pytest

from tests import _gemm_ref64 as G

pytestmark = pytest.mark.gpu

FORMS = {"default": {}, "splitk0": {"X3_SPLITK": 0}, "splitk1": {"X3_SPLITK": 1},
         "exact": {"GEMM_EXACT": 1}, "queue": {"X3P_QUEUE": 1}}
SLICE_ROWS = [0, 64, 192, 4096]
SHAPES = [(16, 16), (32, 64), (64, 64), (48, 80), (128, 128), (32, 272), (144, 16)]
ROWS = [1, 63, 64, 65, 127, 129, 1031, 4099]
OPTIONS = [("relu_mask",), ("colsum",), ("binarize", "colsum"), ("b_row_scale",), ("c_scale",),
           ("b_drop",), ("b_drop", "b_row_scale"), ("relu_mask", "colsum", "c_scale")]
both = pytest.mark.parametrize("form,slice_rows", [(f, r) for f in FORMS for r in SLICE_ROWS])


@pytest.fixture(scope="module")
def lib():
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    return nat.load()


@pytest.fixture(scope="module")
def big():
    """The 70,001-row cases and their float64 references, computed once for the module."""
    out = {}
    for M in (64, 128):
        f = G.make_tn_case(70_001 + M, 70_001, M, M, opts=("colsum",))
        out[M] = (f, G.tn_ref64(f))
    return out


def _run(lib, dev, form, slice_rows, cases, lds=None, refs=None, what=""):
    """One call under (form, slice_rows): checks every member against float64 and, for a fixed
    slice length, the workspace size against the header's formula. Returns the outputs."""
    with G.tuning(lib, **FORMS[form], SPLITK_ROWS=slice_rows):
        outs, need = G.launch_tn(lib, dev, cases, lds)
    if slice_rows:
        want = sum(G.tn_workspace_bytes(f["rows"], f["M"], f["N"], f.get("colsum"), slice_rows)
                   for f in cases)
        assert need == want, (what, need, want)
    for i, (f, o) in enumerate(zip(cases, outs)):
        G.check_tn_case(f, o, refs[i] if refs else None,
                        what=f"{form} slice {slice_rows} {what} member {i} rows {f['rows']} "
                             f"M {f['M']} N {f['N']} {f['opts']}")
    return outs


def _same(a, b):
    return np.array_equal(a["C_bits"], b["C_bits"]) and (
        "colsum_bits" not in a or np.array_equal(a["colsum_bits"], b["colsum_bits"]))


@both
def test_shapes(dev, lib, form, slice_rows):
    """Every (M, N) x rows; colsum_A on every second case. The producer-wave kernel takes the
    4,099-row 64 x 64 and 128 x 128 cases: two runs bitwise equal, and the queue form bitwise
    the barrier form."""
    for j, (M, N) in enumerate(SHAPES):
        for rows in ROWS:
            f = G.make_tn_case(rows + M + N, rows, M, N, opts=("colsum",) if (j + rows) % 2 else ())
            (a,) = _run(lib, dev, form, slice_rows, [f], what="shape")
            if rows in (129, 4099):
                (b,) = _run(lib, dev, form, slice_rows, [f], what="shape again")
                assert _same(a, b), (form, slice_rows, M, N, rows, "two runs differ")
            if form == "queue" and rows == 4099:
                (c,) = _run(lib, dev, "default", slice_rows, [f], what="barrier form")
                assert _same(a, c), (slice_rows, M, N, "queue form differs from the barrier form")


@both
def test_leading_dimensions(dev, lib, form, slice_rows):
    for M, N, rows in ((48, 80, 129), (64, 64, 4099), (128, 128, 4099)):
        f = G.make_tn_case(rows + M, rows, M, N, opts=("relu_mask", "colsum"))
        for pad in (4, 16):
            _run(lib, dev, form, slice_rows, [f], [dict(lda=pad, ldb=pad, ldm=pad)],
                 what=f"ld + {pad}")


@both
def test_options(dev, lib, form, slice_rows):
    """Each option alone and the callers' combinations, at a ragged f32-tile shape, a
    producer-wave shape and a wide one."""
    for opts in OPTIONS:
        for M, N, rows in ((48, 80, 129), (64, 64, 4099), (32, 272, 1031)):
            _run(lib, dev, form, slice_rows, [G.make_tn_case(len(opts) + rows, rows, M, N, opts)],
                 what="option")


@pytest.mark.parametrize("rows", [(300, 17), (70_001, 33), (0, 65), (65, 0), (0, 0)])
@both
def test_groups(dev, lib, form, slice_rows, rows, big):
    """Two products in one launch: an empty member's C and colsum_A come back as exact zeros
    (the float64 reference of an empty product, magnitude 0), the live one right."""
    cases, refs = [], []
    for i, r in enumerate(rows):
        f = big[64][0] if r == 70_001 else G.make_tn_case(7 * i + r, r, 64, 64, opts=("colsum",))
        cases.append(f)
        refs.append(big[64][1] if r == 70_001 else None)
    a = _run(lib, dev, form, slice_rows, cases, refs=refs, what=f"group {rows}")
    if rows == (70_001, 33):
        b = _run(lib, dev, form, slice_rows, cases, refs=refs, what=f"group {rows} again")
        assert all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("M", [64, 128])
@both
def test_many_slices(dev, lib, form, slice_rows, M, big):
    """70,001 rows: up to 1,094 slices summed in slice order; two runs bitwise equal, the queue
    form bitwise the barrier form."""
    f, ref = big[M]
    (a,) = _run(lib, dev, form, slice_rows, [f], refs=[ref], what="many slices")
    other = "default" if form == "queue" else form
    (b,) = _run(lib, dev, other, slice_rows, [f], refs=[ref], what="many slices again")
    assert _same(a, b), (form, slice_rows, M)


@both
def test_workspace_one_byte_short(dev, lib, form, slice_rows):
    """One byte less than hgd_gemm_tn_workspace_size: HGD_ERR_WORKSPACE, C and colsum_A
    untouched."""
    f = G.make_tn_case(3, 1031, 48, 80, opts=("colsum",))
    with G.tuning(lib, **FORMS[form], SPLITK_ROWS=slice_rows):
        (out,), need = G.launch_tn(lib, dev, [f], short=1, expect=4)
    assert need > 0
    assert (out["C_bits"] == G.SENTINEL).all() and (out["colsum_bits"] == G.SENTINEL).all()
