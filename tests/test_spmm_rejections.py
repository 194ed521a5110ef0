"""CPU: what the eight SpMM hop entry points answer to a call they reject (argument validation
only: every case returns before the first HIP call, so the pointers are small fake integers and
no device is needed). Each case pins the exact hgd_status and the exact error text, including
which message wins when a call has two faults. The expected answers were recorded from the
library before the hop's host launcher took a request struct; they are not derived from the
code under test."""
import pytest

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, BF16 = _native.DT_F32, _native.DT_BF16
P = 16  # a fake, 16-byte aligned, never dereferenced pointer

HEAD = ["rowptr", "col", "val", "row_scale", "n_rows", "n_src_rows", "row_begin", "row_end"]
MHEAD = ["rowptr", "col", "val", "mask", "keep"] + HEAD[3:]
XY = ["X", "ldx", "Y", "ldy", "d"]
XY_DT = ["X", "x_dtype", "ldx", "Y", "y_dtype", "ldy", "d"]
ACT = ["epilogue", "slope"]
PLAN = ["plan", "workspace", "workspace_bytes"]
ORDER = {
    "hgd_spmm": HEAD + XY + ACT + PLAN + ["stream"],
    "hgd_spmm_ordered": HEAD + XY + ACT + PLAN + ["out_row", "stream"],
    "hgd_spmm_blocked": HEAD + XY + ACT + ["n_blocks", "stream"],
    "hgd_spmm_fused": HEAD + XY + ["epi"] + PLAN + ["stream"],
    "hgd_spmm_masked": MHEAD + XY + ACT + PLAN + ["stream"],
    "hgd_spmm_masked_fused": MHEAD + XY + ["epi"] + PLAN + ["stream"],
    "hgd_spmm_dt": HEAD + XY_DT + ACT + PLAN + ["stream"],
    "hgd_spmm_masked_dt": MHEAD + XY_DT + ACT + PLAN + ["stream"],
}
ALL = list(ORDER)
PLAIN = [f for f in ALL if "fused" not in f]
# (the blocked hop takes no plan, and the ordered one refuses split rows before it reads them)
PLAN_CHECKED = [f for f in ALL if f not in ("hgd_spmm_blocked", "hgd_spmm_ordered")]
FUSED = ["hgd_spmm_fused", "hgd_spmm_masked_fused"]
MASKED = ["hgd_spmm_masked", "hgd_spmm_masked_fused", "hgd_spmm_masked_dt"]

# a call every entry point would launch; each case below breaks it somewhere
VALID = dict(rowptr=P, col=P, val=None, row_scale=None, n_rows=3, n_src_rows=2, row_begin=0,
             row_end=3, X=P, ldx=64, Y=P, ldy=64, d=64, epilogue=0, slope=0.0, plan=None,
             workspace=None, workspace_bytes=0, stream=None, mask=P, keep=0.5, x_dtype=BF16,
             y_dtype=BF16, epi={}, n_blocks=2, out_row=P)
NULLS = dict(rowptr=None, col=None, X=None, Y=None, mask=None, out_row=None)
EMPTY = dict(NULLS, row_begin=0, row_end=0)  # all-null call over an empty range
SPLIT = dict(threshold=8, chunk=4, n_heavy=1, n_chunks=2, heavy_rows=P, heavy_cptr=P,
             chunk_heavy=P)  # a complete split plan: 2 chunks × 64 columns × 4 B = 512 B
SEGMENTED = dict(flags=1)
NO_ORDER_PLAN = "no split rows or segmented walk with a row order"
LN_LIMIT = "layer_norm needs d <= 256 (16-byte aligned rows) or d <= 64 "
DT_CODES = "HGD_DT_F32 or HGD_DT_BF16"

CASES = []  # (entry point, overrides of VALID, status, error text)


def case(fns, over, status, text, name=None):
    """The same broken call through each of fns; name: the entry point the message names
    (default: the one called)."""
    for fn in [fns] if isinstance(fns, str) else fns:
        CASES.append((fn, over, status, f"{name or fn}: {text}" if text else ""))


# every entry point: the shared checks, in the order they run
case(ALL, dict(d=0), INVALID, "d must be > 0 (got 0)")
case(ALL, dict(d=-4), INVALID, "d must be > 0 (got -4)")
case(ALL, dict(n_src_rows=-1), INVALID, "negative sizes")
case(ALL, dict(n_rows=-3, row_end=0), INVALID, "negative sizes")
case(ALL, dict(row_end=4), INVALID, "row range [0,4) outside [0,3)")
case(ALL, dict(row_begin=-1), INVALID, "row range [-1,3) outside [0,3)")
case(ALL, dict(row_begin=2, row_end=1), INVALID, "row range [2,1) outside [0,3)")
case(ALL, dict(ldx=63), INVALID, "ldx/ldy must be >= d")
case(ALL, dict(ldy=63), INVALID, "ldx/ldy must be >= d")
case(ALL, dict(Y=None), INVALID, "null rowptr/Y")
case(ALL, dict(X=None), INVALID, "null X")
case([f for f in ALL if f != "hgd_spmm_blocked"], dict(rowptr=None), INVALID, "null rowptr/Y")
case(ALL, dict(d=0, n_src_rows=-1, row_end=4, ldx=-1, Y=None), INVALID, "d must be > 0 (got 0)")
case(ALL, dict(n_src_rows=-1, row_end=4, ldx=63, Y=None), INVALID, "negative sizes")
case(ALL, dict(row_end=4, ldx=63, Y=None), INVALID, "row range [0,4) outside [0,3)")
case(ALL, dict(ldx=63, Y=None, X=None), INVALID, "ldx/ldy must be >= d")
case(ALL, dict(Y=None, X=None), INVALID, "null rowptr/Y")

# an all-null call over an empty range: nothing to launch, unless the entry point's own check
# comes first (the ordered hop's answer to an empty range inside the rows is further down)
UNORDERED = [f for f in ALL if f != "hgd_spmm_ordered"]
case(UNORDERED, EMPTY, OK, "")
case(UNORDERED, dict(NULLS, row_begin=2, row_end=2), OK, "")
case("hgd_spmm_ordered", EMPTY, INVALID, "null out_row")
case("hgd_spmm_ordered", dict(EMPTY, n_rows=0), OK, "")
case("hgd_spmm_ordered", dict(EMPTY, n_rows=0, plan=SEGMENTED), OK, "")
case(FUSED, dict(EMPTY, epi=None), INVALID, "null epilogue descriptor")

# the activation code
case(PLAIN, dict(epilogue=3), INVALID, "bad epilogue 3")
case(PLAIN, dict(epilogue=-1), INVALID, "bad epilogue -1")
case(PLAIN, dict(epilogue=3, Y=None), INVALID, "bad epilogue 3")
case(PLAIN, dict(epilogue=3, ldx=63), INVALID, "ldx/ldy must be >= d")
case(FUSED, dict(epi=dict(act=3)), INVALID, "bad epilogue 3")

# split plan and workspace
case(PLAN_CHECKED, dict(plan=dict(SPLIT, chunk=0)), INVALID, "incomplete split plan")
case(PLAN_CHECKED, dict(plan=dict(SPLIT, heavy_cptr=None)), INVALID, "incomplete split plan")
case(PLAN_CHECKED, dict(plan=SPLIT, workspace=P, workspace_bytes=511), WORKSPACE,
     "workspace 511 < required 512")
case(PLAN_CHECKED, dict(plan=SPLIT, workspace=None, workspace_bytes=512), WORKSPACE,
     "workspace 512 < required 512")
case(PLAN_CHECKED, dict(plan=dict(SPLIT, chunk=0), Y=None), INVALID, "null rowptr/Y")

# the fused row epilogue
case(FUSED, dict(epi=None), INVALID, "null epilogue descriptor")
case(FUSED, dict(epi=None, d=0), INVALID, "null epilogue descriptor")
case(FUSED, dict(epi=dict(act=1, slope=-0.5)), INVALID,
     "a fused activation needs slope >= 0 (got -0.5)")
case(FUSED, dict(epi=dict(layer_norm=2)), INVALID, "layer_norm must be 0/1")
case(FUSED, dict(epi=dict(res1=P, ld_res1=63)), INVALID, "ld_res1 < d")
case(FUSED, dict(epi=dict(res2=P, ld_res2=63)), INVALID, "ld_res2 < d")
case(FUSED, dict(epi=dict(act_out=P, ld_act=63)), INVALID, "ld_act < d")
case(FUSED, dict(epi=dict(sum_out=P, ld_sum_out=64)), INVALID,
     "sum_out and sum_res go together")
case(FUSED, dict(epi=dict(sum_out=P, ld_sum_out=63, sum_res=P, ld_sum_res=64)), INVALID,
     "ld_sum_out / ld_sum_res < d")
case(FUSED, dict(epi=dict(layer_norm=1), d=260, ldx=260, ldy=260), UNSUPPORTED,
     LN_LIMIT + "(got d=260)")
case(FUSED, dict(epi=dict(layer_norm=1), d=65, ldx=65, ldy=65), UNSUPPORTED,
     LN_LIMIT + "(got d=65, unaligned)")
case(FUSED, dict(epi=dict(layer_norm=2, res1=P, ld_res1=63), ldx=63), INVALID,
     "ldx/ldy must be >= d")
case(FUSED, dict(epi=dict(layer_norm=2, res1=P, ld_res1=63), Y=None), INVALID,
     "layer_norm must be 0/1")
case(FUSED, dict(epi=dict(layer_norm=1), d=260, ldx=260, ldy=260, plan=dict(SPLIT, chunk=0)),
     INVALID, "incomplete split plan")

# the edge-dropped view
case(MASKED, dict(keep=0.0), INVALID, "keep must be > 0 (got 0)")
case(MASKED, dict(keep=-0.5), INVALID, "keep must be > 0 (got -0.5)")
case(MASKED, dict(mask=None), INVALID, "null mask")
case(MASKED, dict(keep=0.0, mask=None), INVALID, "keep must be > 0 (got 0)")
case(MASKED, dict(keep=0.0, row_end=4), INVALID, "keep must be > 0 (got 0)")
case(MASKED, dict(EMPTY, keep=0.0), INVALID, "keep must be > 0 (got 0)")
case(MASKED, dict(mask=None, d=0), INVALID, "null mask")
case(MASKED, dict(mask=None, row_begin=3, d=0), INVALID, "d must be > 0 (got 0)")
case("hgd_spmm_masked_fused", dict(epi=None, keep=0.0, mask=None), INVALID,
     "null epilogue descriptor")

# dtype codes; f32 → f32 is the fp32 entry point's call, and says so
DT = ["hgd_spmm_dt", "hgd_spmm_masked_dt"]
for fn in DT:
    case(fn, dict(x_dtype=2), INVALID, f"unknown dtype code (x 2, y 1): {DT_CODES}")
    case(fn, dict(y_dtype=-1, d=0), INVALID, f"unknown dtype code (x 1, y -1): {DT_CODES}")
    case(fn, dict(x_dtype=F32, d=0), INVALID, "d must be > 0 (got 0)")
    case(fn, dict(y_dtype=F32, ldy=63), INVALID, "ldx/ldy must be >= d")
    f32 = fn[:-3]
    both = dict(x_dtype=F32, y_dtype=F32)
    case(fn, dict(both, d=0), INVALID, "d must be > 0 (got 0)", name=f32)
    case(fn, dict(both, d=-4), INVALID, "d must be > 0 (got -4)", name=f32)
    case(fn, dict(both, epilogue=3), INVALID, "bad epilogue 3", name=f32)
    case(fn, dict(both, plan=SPLIT, workspace=P, workspace_bytes=511), WORKSPACE,
         "workspace 511 < required 512", name=f32)
    case(fn, dict(both, **EMPTY), OK, "")
case("hgd_spmm_masked_dt", dict(x_dtype=F32, y_dtype=F32, keep=0.0), INVALID,
     "keep must be > 0 (got 0)", name="hgd_spmm_masked")
case("hgd_spmm_masked_dt", dict(x_dtype=F32, y_dtype=F32, mask=None), INVALID, "null mask",
     name="hgd_spmm_masked")
case("hgd_spmm_masked_dt", dict(x_dtype=2, keep=0.0), INVALID,
     f"unknown dtype code (x 2, y 1): {DT_CODES}")

# source blocks
BLK = "hgd_spmm_blocked"
case(BLK, dict(n_blocks=0), INVALID, "blocks must be 1..64")
case(BLK, dict(n_blocks=65), INVALID, "blocks must be 1..64")
case(BLK, dict(n_blocks=-1), INVALID, "blocks must be 1..64")
case(BLK, dict(rowptr=None), INVALID, "null blk_start")
case(BLK, dict(n_blocks=0, rowptr=None, d=0), INVALID, "blocks must be 1..64")
case(BLK, dict(rowptr=None, d=0), INVALID, "null blk_start")
case(BLK, dict(EMPTY, n_blocks=65), INVALID, "blocks must be 1..64")

# the row order
ORD = "hgd_spmm_ordered"
ALL_ROWS = "a row order covers all rows, got "
case(ORD, dict(out_row=None), INVALID, "null out_row")
case(ORD, dict(out_row=None, d=0), INVALID, "null out_row")
case(ORD, dict(plan=SPLIT, workspace=P, workspace_bytes=512), UNSUPPORTED, NO_ORDER_PLAN)
case(ORD, dict(plan=dict(SPLIT, chunk=0)), UNSUPPORTED, NO_ORDER_PLAN)
case(ORD, dict(plan=SEGMENTED), UNSUPPORTED, NO_ORDER_PLAN)
case(ORD, dict(row_begin=1), UNSUPPORTED, ALL_ROWS + "[1,3) of 3")
case(ORD, dict(row_end=2), UNSUPPORTED, ALL_ROWS + "[0,2) of 3")
case(ORD, dict(row_begin=5, row_end=5), INVALID, "row range [5,5) outside [0,3)")
case(ORD, dict(n_rows=8, row_begin=5, row_end=5), UNSUPPORTED, ALL_ROWS + "[5,5) of 8")
case(ORD, dict(NULLS, out_row=P, row_begin=2, row_end=2), UNSUPPORTED,
     ALL_ROWS + "[2,2) of 3")
case(ORD, dict(plan=SPLIT, d=0), INVALID, "d must be > 0 (got 0)")
case(ORD, dict(plan=SEGMENTED, epilogue=3), INVALID, "bad epilogue 3")
case(ORD, dict(plan=SEGMENTED, row_begin=1), UNSUPPORTED, NO_ORDER_PLAN)
case(ORD, dict(plan=SEGMENTED, Y=None), INVALID, "null rowptr/Y")
case(ORD, dict(row_begin=1, X=None), INVALID, "null X")


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


def test_every_entry_point_and_feature_is_covered():
    assert {c[0] for c in CASES} == set(ALL) and len(CASES) > 250
    # nothing here may reach a launch: an accepted call has no rows to run
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
    del keep


def test_accepted_call_clears_the_error_text():
    """An earlier failure's text does not survive the next call (and none is left behind for
    later tests that read hgd_get_last_error_string)."""
    lib = _native.load()
    for fn in ALL:
        bad, _k = make_args(fn, dict(d=0))
        assert getattr(lib, fn)(*bad) == INVALID
        assert lib.hgd_get_last_error_string() != b""
        good, _k = make_args(fn, dict(EMPTY, n_rows=0))
        assert getattr(lib, fn)(*good) == OK
        assert lib.hgd_get_last_error_string() == b""
