"""hgd_gemm_rows at every kernel form against float64 (tests/_gemm_ref64.py): the staged
split-bf16 kernel at each HGD_TUNE_X3S_TILES, the unstaged split-bf16 kernel (HGD_TUNE_X3_COLS),
the f32-MFMA kernel (HGD_TUNE_GEMM_EXACT, and every call the others hand to it: K % 32 != 0,
output rows that are not 16-byte aligned) — all K, N up to 272 (several column slices, ragged
last slice, workgroups without a tile), row edges, the persistent loop, leading dimensions above
the width, every epilogue, groups with empty and very unequal members, and bitwise properties.
Every call runs in sentinel-guarded buffers: nothing outside [rows, width] may change."""
import numpy as np
import pytest

from tests import _gemm_ref64 as G

pytestmark = pytest.mark.gpu

FORMS = {"default": {}, "tiles1": {"X3S_TILES": 1}, "tiles2": {"X3S_TILES": 2},
         "tiles3": {"X3S_TILES": 3}, "cols64": {"X3_COLS": 64}, "cols128": {"X3_COLS": 128},
         "exact": {"GEMM_EXACT": 1}}
KS = [16, 32, 48, 64, 80, 96, 112, 128]
NS = [16, 32, 48, 64, 80, 128, 144, 192, 272]
EPILOGUES = {"accumulate": ("accumulate",), "res": ("res",), "relu_mask": ("relu_mask",),
             "relu_mask_accumulate": ("relu_mask", "accumulate"),
             "binarize_row_inv": ("binarize_row_inv",), "b_row_count": ("b_row_count",),
             "b_scale": ("b_scale",), "drop": ("drop",), "a_drop": ("a_drop",),
             "a_drop_res": ("a_drop", "res"), "relu_mask_drop": ("relu_mask", "drop")}
_skipped = []  # share of elements the ReLU sign filter skipped, one entry per compared case


@pytest.fixture(scope="module")
def lib():
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    yield nat.load()
    if _skipped:
        print(f"\nReLU sign filter: skipped share max {max(_skipped):.2e} over "
              f"{len(_skipped)} cases")


def _run(lib, dev, form, cases, lds=None, what="", **extra):
    with G.tuning(lib, **FORMS[form], **extra):
        outs = G.launch_rows(lib, dev, cases, lds)
    for i, (f, o) in enumerate(zip(cases, outs)):
        G.check_rows_case(f, o, exact=form == "exact", stats=_skipped,
                          what=f"{form} {what} member {i} rows {f['rows']} K {f['K']} N {f['N']} "
                               f"{f['orient']} {f['opts']}")
    return outs


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("form", FORMS)
def test_width_matrix(dev, lib, form, K):
    """rows = 257 (16 full tiles and a one-row tail), every N, bias + ReLU, both B orientations
    with ldw = width + 16."""
    for N in NS:
        for orient in ("fwd", "bwd"):
            _run(lib, dev, form, [G.make_rows_case(K * 1000 + N, 257, K, N, orient)], what="width")


@pytest.mark.parametrize("K,N", [(32, 64), (64, 48), (128, 144)])
@pytest.mark.parametrize("form", FORMS)
def test_row_edges(dev, lib, form, K, N):
    for rows in (1, 15, 16, 17, 63, 64, 65, 1031):
        _run(lib, dev, form, [G.make_rows_case(rows + K, rows, K, N, "fwd")], what="row edge")


@pytest.fixture(scope="module")
def big_case():
    f = G.make_rows_case(70_001, 70_001, 64, 144, "fwd")
    f["cache_ref"] = True  # always laid out the same way: one float64 reference for all tests
    return f


@pytest.mark.parametrize("form", FORMS)
def test_persistent_loop(dev, lib, form, big_case):
    """70,001 rows: every form's capped grid walks several tiles (stages) per wave."""
    _run(lib, dev, form, [big_case], what="persistent")


def test_persistent_loop_f32_64_blocks(dev, lib):
    """The f32 form under HGD_TUNE_ROWGEMM_BLOCKS = 64 at 8,209 rows: two full rounds of
    64 blocks x 4 waves x 16 rows and a ragged third."""
    _run(lib, dev, "exact", [G.make_rows_case(8209, 8209, 64, 144, "fwd")], what="64 blocks",
         ROWGEMM_BLOCKS=64)


@pytest.mark.parametrize("K,N", [(32, 64), (64, 144)])
@pytest.mark.parametrize("form", FORMS)
def test_leading_dimensions_and_alignment(dev, lib, form, K, N):
    """rows = 65: lda, ldm, ldy, ldres, ldy2 = width + 4 and + 16; then Y / Y2 rows that are not
    16-byte aligned (ldy = N + 1, and a base 4 bytes off), which must run on the f32 kernel —
    bitwise what HGD_TUNE_GEMM_EXACT = 1 gives on the same layout — with the padding intact."""
    for opts in ((), ("res",), ("relu_mask",), ("accumulate",)):
        orient = "bwd" if "relu_mask" in opts else "fwd"
        f = G.make_rows_case(65 + K, 65, K, N, orient, opts=opts)
        for pad in (4, 16):
            _run(lib, dev, form, [f], [dict(lda=pad, ldm=pad, ldy=pad, ldres=pad, ldy2=pad)],
                 what=f"ld + {pad}")
        for ld in (dict(ldy=1, ldy2=1), dict(y_off=1), dict(lda=4, ldres=4, ldy=1, ldy2=5)):
            (got,) = _run(lib, dev, form, [f], [ld], what=f"unaligned {ld}")
            (exact,) = _run(lib, dev, "exact", [f], [ld], what=f"unaligned {ld}")
            assert np.array_equal(got["Y_bits"], exact["Y_bits"]), (form, opts, ld)
            if "Y2" in got:
                assert np.array_equal(got["Y2"].view(np.int32), exact["Y2"].view(np.int32))


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("form", FORMS)
def test_epilogues(dev, lib, form, epi):
    """Each epilogue alone and the combinations the callers use; row_inv is compared too (one
    value per row, its neighbours in the guarded buffer untouched, also at N > 128 where three
    column slices see the row)."""
    opts = EPILOGUES[epi]
    orient = "bwd" if "relu_mask" in opts else "fwd"
    for rows in (17, 257):
        for K, N in ((32, 32), (64, 64), (128, 144)):
            _run(lib, dev, form, [G.make_rows_case(rows + K + N, rows, K, N, orient, opts=opts)],
                 what=epi)


@pytest.mark.parametrize("rows", [(300, 17), (17, 300), (70_001, 33), (0, 65), (65, 0), (0, 0)])
@pytest.mark.parametrize("form", FORMS)
def test_groups(dev, lib, form, rows, big_case):
    """Two products in one launch, each against float64 on its own: unequal members (the small
    one's share of a capped grid rounds to the minimum), an empty first / second / both."""
    K, N = 64, 144
    cases = [big_case if r == 70_001 else G.make_rows_case(11 * i + r, r, K, N, "fwd")
             for i, r in enumerate(rows)]
    _run(lib, dev, form, cases, what=f"group {rows}")
    if rows == (300, 17):  # and a narrow group with a residual on both members
        cases = [G.make_rows_case(5 + i, r, 32, 48, "fwd", opts=("res",))
                 for i, r in enumerate(rows)]
        _run(lib, dev, form, cases, what="group res")


@pytest.mark.parametrize("form", FORMS)
def test_group_rejects_mismatched_epilogues(dev, lib, form):
    """accumulate on one member and a residual on the other: HGD_ERR_INVALID_ARG under every
    form, and nothing written."""
    a = G.make_rows_case(1, 65, 64, 64, "fwd", opts=("accumulate",))
    b = G.make_rows_case(2, 65, 64, 64, "fwd", opts=("res",))
    with G.tuning(lib, **FORMS[form]):
        outs = G.launch_rows(lib, dev, [a, b], expect=1)
    assert np.array_equal(outs[0]["Y_bits"], a["Y_in"].view(np.int32))
    assert (outs[1]["Y_bits"] == G.SENTINEL).all()
    assert (outs[1]["Y2"].view(np.int32) == G.SENTINEL).all()


def _slice(f, a, b):
    g = dict(f)
    g["A"], g["rows"] = f["A"][a:b], b - a
    return g


@pytest.mark.parametrize("K,N", [(64, 64), (128, 144)])
@pytest.mark.parametrize("form", FORMS)
def test_bitwise_row_independence(dev, lib, form, K, N):
    """A row's result depends only on its own A row, B and the epilogue operands: at 1,031 rows
    the plain call equals, bit for bit, the call under another grid cap, the same product as the
    second member of a group, and the concatenation of calls on row slices."""
    f = G.make_rows_case(K + N, 1031, K, N, "fwd")
    base = _run(lib, dev, form, [f])[0]["Y_bits"]
    for blocks in (64, 8192):
        got = _run(lib, dev, form, [f], ROWGEMM_BLOCKS=blocks)[0]["Y_bits"]
        assert np.array_equal(got, base), f"ROWGEMM_BLOCKS = {blocks}"
    other = G.make_rows_case(99, 300, K, N, "fwd")
    got = _run(lib, dev, form, [other, f])[1]["Y_bits"]
    assert np.array_equal(got, base), "second member of a group"
    for cut in (512, 37):
        parts = [_run(lib, dev, form, [_slice(f, a, b)])[0]["Y_bits"]
                 for a, b in ((0, cut), (cut, 1031))]
        assert np.array_equal(np.concatenate(parts), base), f"row slices at {cut}"
