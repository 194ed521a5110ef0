"""CPU: what the ordered twins of the fused, masked and 16-bit hops answer to a call they refuse
(argument validation only: every case returns before the first HIP call — this machine has no
device, so a launch would not come back as one of these statuses — the pointers are small fake
integers). Each case pins the hgd_status and the exact error text, which starts with the name of
the entry point called.

A row order still excludes split rows, the segmented walk and a row range other than all rows,
and a fused LayerNorm row must fit one column pass as without an order. (Source blocks with a
mask or a row epilogue stay refused inside the launcher, spmm_check_args; no entry point takes
source blocks together with either, so no call can ask for it.)"""
import pytest

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, UNSUPPORTED = 0, 1, 3
F32, BF16 = _native.DT_F32, _native.DT_BF16
P = 16  # a fake, 16-byte aligned, never dereferenced pointer

HEAD = ["rowptr", "col", "val", "row_scale", "n_rows", "n_src_rows", "row_begin", "row_end"]
MHEAD = ["rowptr", "col", "val", "mask", "keep"] + HEAD[3:]
XY = ["X", "ldx", "Y", "ldy", "d"]
XY_DT = ["X", "x_dtype", "ldx", "Y", "y_dtype", "ldy", "d"]
XY_FDT = ["X", "x_dtype", "ldx", "Y", "ldy", "d"]
ACT = ["epilogue", "slope"]
TAIL = ["plan", "workspace", "workspace_bytes", "out_row", "stream"]
ORDER = {
    "hgd_spmm_fused_ordered": HEAD + XY + ["epi"] + TAIL,
    "hgd_spmm_masked_ordered": MHEAD + XY + ACT + TAIL,
    "hgd_spmm_masked_fused_ordered": MHEAD + XY + ["epi"] + TAIL,
    "hgd_spmm_ordered_dt": HEAD + XY_DT + ACT + TAIL,
    "hgd_spmm_masked_ordered_dt": MHEAD + XY_DT + ACT + TAIL,
    "hgd_spmm_fused_ordered_dt": HEAD + XY_FDT + ["epi", "y16", "ld_y16"] + TAIL,
    "hgd_spmm_masked_fused_ordered_dt": MHEAD + XY_FDT + ["epi", "y16", "ld_y16"] + TAIL,
}
ALL = list(ORDER)
FUSED = [f for f in ALL if "fused" in f]
MASKED = [f for f in ALL if "masked" in f]
DT = [f for f in ALL if f.endswith("_dt")]
# the fp32 entry point a _dt one forwards an all-float32 call to, which then answers by its name
F32_TWIN = {"hgd_spmm_ordered_dt": "hgd_spmm_ordered",
            "hgd_spmm_masked_ordered_dt": "hgd_spmm_masked_ordered",
            "hgd_spmm_fused_ordered_dt": "hgd_spmm_fused_ordered",
            "hgd_spmm_masked_fused_ordered_dt": "hgd_spmm_masked_fused_ordered"}

# a call every entry point would launch; each case below breaks it somewhere
VALID = dict(rowptr=P, col=P, val=None, row_scale=None, n_rows=3, n_src_rows=2, row_begin=0,
             row_end=3, X=P, ldx=64, Y=P, ldy=64, d=64, epilogue=0, slope=0.0, plan=None,
             workspace=None, workspace_bytes=0, stream=None, mask=P, keep=0.5, x_dtype=BF16,
             y_dtype=BF16, epi={}, y16=None, ld_y16=0, out_row=P)
NULLS = dict(rowptr=None, col=None, X=None, Y=None, mask=None, out_row=None)
SPLIT = dict(threshold=8, chunk=4, n_heavy=1, n_chunks=2, heavy_rows=P, heavy_cptr=P,
             chunk_heavy=P)
SEGMENTED = dict(flags=1)
NO_ORDER_PLAN = "no split rows or segmented walk with a row order"
ALL_ROWS = "a row order covers all rows, got "
LN_LIMIT = "layer_norm needs d <= 256 (16-byte aligned rows) or d <= 64 "

CASES = []  # (entry point, overrides of VALID, status, error text)


def case(fns, over, status, text, name=None):
    for fn in [fns] if isinstance(fns, str) else fns:
        CASES.append((fn, over, status, f"{name or fn}: {text}" if text else ""))


# the order itself
case(ALL, dict(out_row=None), INVALID, "null out_row")
case(ALL, dict(out_row=None, d=0), INVALID, "null out_row")
case(ALL, dict(NULLS, row_begin=0, row_end=0), INVALID, "null out_row")
case(ALL, dict(NULLS, n_rows=0, row_begin=0, row_end=0), OK, "")
# what a row order excludes, after the checks every hop makes
case(ALL, dict(plan=SPLIT, workspace=P, workspace_bytes=512), UNSUPPORTED, NO_ORDER_PLAN)
case(ALL, dict(plan=dict(SPLIT, chunk=0)), UNSUPPORTED, NO_ORDER_PLAN)
case(ALL, dict(plan=SEGMENTED), UNSUPPORTED, NO_ORDER_PLAN)
case(ALL, dict(row_begin=1), UNSUPPORTED, ALL_ROWS + "[1,3) of 3")
case(ALL, dict(row_end=2), UNSUPPORTED, ALL_ROWS + "[0,2) of 3")
case(ALL, dict(n_rows=8, row_begin=5, row_end=5), UNSUPPORTED, ALL_ROWS + "[5,5) of 8")
case(ALL, dict(plan=SEGMENTED, row_begin=1), UNSUPPORTED, NO_ORDER_PLAN)
case(ALL, dict(plan=SPLIT, d=0), INVALID, "d must be > 0 (got 0)")
case(ALL, dict(plan=SEGMENTED, Y=None), INVALID, "null rowptr/Y")
case(ALL, dict(row_begin=1, X=None), INVALID, "null X")
case(ALL, dict(row_end=4), INVALID, "row range [0,4) outside [0,3)")
# the mask and the epilogue keep their own checks
case(MASKED, dict(mask=None), INVALID, "null mask")
case(MASKED, dict(keep=0.0, row_begin=1), INVALID, "keep must be > 0 (got 0)")
case(MASKED, dict(mask=None, plan=SEGMENTED), INVALID, "null mask")
case(FUSED, dict(epi=None), INVALID, "null epilogue descriptor")
case(FUSED, dict(epi=None, out_row=None), INVALID, "null epilogue descriptor")
case(FUSED, dict(epi=dict(layer_norm=2), row_begin=1), INVALID, "layer_norm must be 0/1")
case(FUSED, dict(epi=dict(res1=P, ld_res1=63)), INVALID, "ld_res1 < d")
# a fused LayerNorm row that does not fit one column pass: as without an order, and after the
# order's own refusals
WIDE = dict(d=264, ldx=264, ldy=264)  # (16-byte rows in both element sizes)
case(FUSED, dict(WIDE, epi=dict(layer_norm=1)), UNSUPPORTED, LN_LIMIT + "(got d=264)")
case(FUSED, dict(epi=dict(layer_norm=1), d=65, ldx=65, ldy=65), UNSUPPORTED,
     LN_LIMIT + "(got d=65, unaligned)")
case(FUSED, dict(WIDE, epi=dict(layer_norm=1), plan=SEGMENTED), UNSUPPORTED, NO_ORDER_PLAN)
case(FUSED, dict(WIDE, epi=dict(layer_norm=1), row_end=2), UNSUPPORTED, ALL_ROWS + "[0,2) of 3")
# dtype codes; an all-float32 call is the fp32 ordered twin's, and says so
for fn in DT:
    fused = "fused" in fn
    codes = "(x 2)" if fused else "(x 2, y 1)"
    case(fn, dict(x_dtype=2, out_row=None), INVALID,
         f"unknown dtype code {codes}: HGD_DT_F32 or HGD_DT_BF16")
    both = dict(x_dtype=F32, y_dtype=F32)
    twin = F32_TWIN[fn]
    case(fn, dict(both, out_row=None), INVALID, "null out_row", name=twin)
    case(fn, dict(both, plan=SEGMENTED), UNSUPPORTED, NO_ORDER_PLAN, name=twin)
    case(fn, dict(both, row_begin=1), UNSUPPORTED, ALL_ROWS + "[1,3) of 3", name=twin)
    if fused:
        case(fn, dict(both, y16=P, ld_y16=64), UNSUPPORTED,
             "y16 needs a bfloat16 table (x HGD_DT_F32)")
        case(fn, dict(y16=P, ld_y16=63), INVALID, "ld_y16 < d")


def make_args(fn, over):
    v = dict(VALID, **over)
    keep = []  # the structs outlive the call
    for key, cls in (("plan", _native.SplitPlan), ("epi", _native.RowEpilogue)):
        if v[key] is not None:
            keep.append(cls(**v[key]))
            v[key] = keep[-1]
    return [v[k] for k in ORDER[fn]], keep


def case_id(c):
    return c[0][4:] + "-" + ",".join(
        f"{k}={sorted(x) if isinstance(x, dict) else x}" for k, x in c[1].items())


def test_every_entry_point_is_covered_and_nothing_reaches_a_launch():
    assert {c[0] for c in CASES} == set(ALL)
    for fn in ALL:
        texts = [c[3] for c in CASES if c[0] == fn and c[3].startswith(fn + ": ")]
        for refusal in ("null out_row", NO_ORDER_PLAN, ALL_ROWS + "[1,3) of 3"):
            assert any(t.endswith(refusal) for t in texts), (fn, refusal)
    # an accepted call has no rows to run
    for fn, over, status, _ in CASES:
        v = dict(VALID, **over)
        assert status != OK or v["row_begin"] == v["row_end"], (fn, over)


@pytest.mark.parametrize("fn,over,status,text", CASES, ids=[case_id(c) for c in CASES])
def test_rejection(fn, over, status, text):
    lib = _native.load()
    args, keep = make_args(fn, over)
    got = getattr(lib, fn)(*args)
    msg = lib.hgd_get_last_error_string().decode()
    print(f"{fn}: status {got}, {msg!r}")
    assert (got, msg) == (status, text)
    if status != OK:
        assert msg.startswith(fn) or msg.startswith(F32_TWIN.get(fn, fn))
    del keep


def test_accepted_call_clears_the_error_text():
    lib = _native.load()
    for fn in ALL:
        bad, _k = make_args(fn, dict(out_row=None))
        assert getattr(lib, fn)(*bad) == INVALID
        assert lib.hgd_get_last_error_string() != b""
        good, _k = make_args(fn, dict(NULLS, n_rows=0, row_begin=0, row_end=0))
        assert getattr(lib, fn)(*good) == OK
        assert lib.hgd_get_last_error_string() == b""
