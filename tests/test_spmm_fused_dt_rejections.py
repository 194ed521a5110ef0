"""CPU: what the fused row epilogue over a bfloat16 table (hgd_spmm_fused_dt /
hgd_spmm_masked_fused_dt) answers to a call it rejects, and the TypeErrors of its Python host
(incidence.spmm_csr_fused_dt, the ``gather_dtype`` of functional.two_hop_fused /
att_two_hop_fused). Argument validation only: every case returns before the first HIP call, so
the pointers are small fake integers and no device is needed (the style of
tests/test_spmm_rejections.py and tests/test_spmm_blocked_dt_rejections.py). Each case pins the
hgd_status and the exact error text."""
import types

import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, BF16 = _native.DT_F32, _native.DT_BF16
P = 16  # a fake, 16-byte aligned, never dereferenced pointer
DT_CODES = "HGD_DT_F32 or HGD_DT_BF16"
LN_LIMIT = "layer_norm needs d <= 256 (16-byte aligned rows) or d <= 64 "

HEAD = ["rowptr", "col", "val", "row_scale", "n_rows", "n_src_rows", "row_begin", "row_end"]
MHEAD = ["rowptr", "col", "val", "mask", "keep"] + HEAD[3:]
TAIL = ["X", "x_dtype", "ldx", "Y", "ldy", "d", "epi", "y16", "ld_y16", "plan", "workspace",
        "workspace_bytes", "stream"]
ORDER = {"hgd_spmm_fused_dt": HEAD + TAIL, "hgd_spmm_masked_fused_dt": MHEAD + TAIL}
BOTH = list(ORDER)
F32_NAME = {"hgd_spmm_fused_dt": "hgd_spmm_fused",
            "hgd_spmm_masked_fused_dt": "hgd_spmm_masked_fused"}

# a call both entry points would launch; each case below breaks it somewhere
VALID = dict(rowptr=P, col=P, val=None, row_scale=None, n_rows=3, n_src_rows=2, row_begin=0,
             row_end=3, X=P, x_dtype=BF16, ldx=64, Y=P, ldy=64, d=64, epi={}, y16=P, ld_y16=64,
             plan=None, workspace=None, workspace_bytes=0, stream=None, mask=P, keep=0.5)
NULLS = dict(rowptr=None, col=None, X=None, Y=None, mask=None, y16=None, ld_y16=0)
EMPTY = dict(NULLS, row_begin=0, row_end=0)  # all-null call over an empty range
SPLIT = dict(threshold=8, chunk=4, n_heavy=1, n_chunks=2, heavy_rows=P, heavy_cptr=P,
             chunk_heavy=P)  # a complete split plan: 2 chunks × 64 columns × 4 B = 512 B (fp32)
# More rows than the widest grid: at d = 64 a lane owns 8 columns, a group is 8 lanes, a
# workgroup 32 rows, so 2^37 rows are 2^32 workgroups. The launcher refuses that grid after every
# argument check and the pass plan and before it launches anything: the answer of an ACCEPTED
# call without a device.
HUGE = dict(n_rows=1 << 37, row_end=1 << 37)
TOO_LARGE = "grid too large"

CASES = []  # (entry point, overrides of VALID, status, error text)


def case(over, status, text, fns=BOTH, f32=False):
    """The same broken call through each of fns; f32: the message names the fp32 entry point
    the call was forwarded to."""
    for fn in [fns] if isinstance(fns, str) else fns:
        name = F32_NAME[fn] if f32 else fn
        CASES.append((fn, over, status, f"{name}: {text}" if text else ""))


# the dtype code comes first
case(dict(x_dtype=2), INVALID, f"unknown dtype code (x 2): {DT_CODES}")
case(dict(x_dtype=-1, d=0, epi=None), INVALID, f"unknown dtype code (x -1): {DT_CODES}")
case(dict(x_dtype=2, keep=0.0), INVALID, f"unknown dtype code (x 2): {DT_CODES}",
     fns="hgd_spmm_masked_fused_dt")
# an fp32 table: a y16 is unsupported; without one the call is the fp32 entry point's, which says so
case(dict(x_dtype=F32), UNSUPPORTED, "y16 needs a bfloat16 table (x HGD_DT_F32)")
case(dict(x_dtype=F32, d=0), UNSUPPORTED, "y16 needs a bfloat16 table (x HGD_DT_F32)")
case(dict(x_dtype=F32, epi=None), UNSUPPORTED, "y16 needs a bfloat16 table (x HGD_DT_F32)")
NO16 = dict(x_dtype=F32, y16=None, ld_y16=0)
case(dict(NO16, epi=None), INVALID, "null epilogue descriptor", f32=True)
case(dict(NO16, d=0), INVALID, "d must be > 0 (got 0)", f32=True)
case(dict(NO16, ldy=63), INVALID, "ldx/ldy must be >= d", f32=True)
case(dict(NO16, epi=dict(layer_norm=2)), INVALID, "layer_norm must be 0/1", f32=True)
case(dict(NO16, plan=SPLIT, workspace=P, workspace_bytes=511), WORKSPACE,
     "workspace 511 < required 512", f32=True)
case(dict(NO16, **EMPTY), OK, "")
case(dict(NO16, keep=0.0), INVALID, "keep must be > 0 (got 0)", fns="hgd_spmm_masked_fused_dt",
     f32=True)
# the descriptor
case(dict(epi=None), INVALID, "null epilogue descriptor")
case(dict(epi=None, d=0), INVALID, "null epilogue descriptor")
case(dict(EMPTY, epi=None), INVALID, "null epilogue descriptor")
case(dict(epi=None, keep=0.0, mask=None), INVALID, "null epilogue descriptor",
     fns="hgd_spmm_masked_fused_dt")
# the shared checks, in the order they run
case(dict(d=0), INVALID, "d must be > 0 (got 0)")
case(dict(d=-4), INVALID, "d must be > 0 (got -4)")
case(dict(n_src_rows=-1), INVALID, "negative sizes")
case(dict(n_rows=-3, row_end=0), INVALID, "negative sizes")
case(dict(row_end=4), INVALID, "row range [0,4) outside [0,3)")
case(dict(row_begin=-1), INVALID, "row range [-1,3) outside [0,3)")
case(dict(row_begin=2, row_end=1), INVALID, "row range [2,1) outside [0,3)")
case(dict(ldx=63), INVALID, "ldx/ldy must be >= d")
case(dict(ldy=63), INVALID, "ldx/ldy must be >= d")
case(dict(Y=None), INVALID, "null rowptr/Y")
case(dict(rowptr=None), INVALID, "null rowptr/Y")
case(dict(X=None), INVALID, "null X")
case(EMPTY, OK, "")
case(dict(NULLS, row_begin=2, row_end=2), OK, "")
# the fused row epilogue's own, and the bf16 copy's leading dimension after them
case(dict(epi=dict(act=3)), INVALID, "bad epilogue 3")
case(dict(epi=dict(act=1, slope=-0.5)), INVALID, "a fused activation needs slope >= 0 (got -0.5)")
case(dict(epi=dict(layer_norm=2)), INVALID, "layer_norm must be 0/1")
case(dict(epi=dict(res1=P, ld_res1=63)), INVALID, "ld_res1 < d")
case(dict(epi=dict(res2=P, ld_res2=63)), INVALID, "ld_res2 < d")
case(dict(epi=dict(act_out=P, ld_act=63)), INVALID, "ld_act < d")
case(dict(epi=dict(sum_out=P, ld_sum_out=64)), INVALID, "sum_out and sum_res go together")
case(dict(epi=dict(sum_out=P, ld_sum_out=63, sum_res=P, ld_sum_res=64)), INVALID,
     "ld_sum_out / ld_sum_res < d")
case(dict(ld_y16=63), INVALID, "ld_y16 < d")
case(dict(ld_y16=0), INVALID, "ld_y16 < d")
case(dict(ld_y16=-8), INVALID, "ld_y16 < d")
case(dict(ld_y16=63, epi=dict(res1=P, ld_res1=63)), INVALID, "ld_res1 < d")
case(dict(ld_y16=63, ldx=63), INVALID, "ldx/ldy must be >= d")
case(dict(ld_y16=63, Y=None), INVALID, "ld_y16 < d")
case(dict(y16=None, ld_y16=0, Y=None), INVALID, "null rowptr/Y")  # no copy: its ld is not read
# LayerNorm needs the row in one lane group: 256 columns of 8-column lanes, 64 of one-column
# lanes; the bf16 copy takes part in the 16-byte test like the side tables
case(dict(epi=dict(layer_norm=1), d=264, ldx=264, ldy=264, ld_y16=264), UNSUPPORTED,
     LN_LIMIT + "(got d=264)")
case(dict(epi=dict(layer_norm=1), d=68, ldx=68, ldy=68, ld_y16=68), UNSUPPORTED,
     LN_LIMIT + "(got d=68, unaligned)")  # d % 8 != 0
case(dict(epi=dict(layer_norm=1), d=72, ldx=72, ldy=72, ld_y16=73), UNSUPPORTED,
     LN_LIMIT + "(got d=72, unaligned)")
case(dict(epi=dict(layer_norm=1), d=72, ldx=72, ldy=72, ld_y16=72, y16=P + 2), UNSUPPORTED,
     LN_LIMIT + "(got d=72, unaligned)")
case(dict(epi=dict(layer_norm=1), d=72, ldx=76, ldy=72, ld_y16=72), UNSUPPORTED,
     LN_LIMIT + "(got d=72, unaligned)")  # ldx % 8 != 0: bf16 rows off the 16-byte grid
# the workspace of the split rows: hgd_spmm_workspace_size's fp32 partials, unchanged
case(dict(plan=dict(SPLIT, chunk=0)), INVALID, "incomplete split plan")
case(dict(plan=dict(SPLIT, heavy_cptr=None)), INVALID, "incomplete split plan")
case(dict(plan=SPLIT, workspace=P, workspace_bytes=511), WORKSPACE,
     "workspace 511 < required 512")
case(dict(plan=SPLIT, workspace=None, workspace_bytes=512), WORKSPACE,
     "workspace 512 < required 512")
case(dict(plan=dict(SPLIT, chunk=0), Y=None), INVALID, "null rowptr/Y")
# the edge-dropped view
MASKED = "hgd_spmm_masked_fused_dt"
case(dict(keep=0.0), INVALID, "keep must be > 0 (got 0)", fns=MASKED)
case(dict(keep=-0.5), INVALID, "keep must be > 0 (got -0.5)", fns=MASKED)
case(dict(mask=None), INVALID, "null mask", fns=MASKED)
case(dict(keep=0.0, mask=None), INVALID, "keep must be > 0 (got 0)", fns=MASKED)
case(dict(EMPTY, keep=0.0), INVALID, "keep must be > 0 (got 0)", fns=MASKED)
case(dict(mask=None, d=0), INVALID, "null mask", fns=MASKED)
# accepted: everything passes and only the grid is refused — with and without the bf16 copy,
# LayerNorm at the widest row, a fused row wider than 256 columns without LayerNorm (256-column
# passes of 32 lanes: 8 rows per workgroup), the scalar path, a segmented plan (walked by rows)
case(HUGE, UNSUPPORTED, TOO_LARGE)
case(dict(HUGE, y16=None, ld_y16=0), UNSUPPORTED, TOO_LARGE)
case(dict(HUGE, epi=dict(layer_norm=1), d=256, ldx=256, ldy=256, ld_y16=256), UNSUPPORTED,
     TOO_LARGE)
case(dict(HUGE, d=512, ldx=512, ldy=512, ld_y16=512), UNSUPPORTED, TOO_LARGE)
case(dict(HUGE, epi=dict(layer_norm=1), d=5, ldx=5, ldy=5, ld_y16=5), UNSUPPORTED, TOO_LARGE)
case(dict(HUGE, plan=dict(flags=1)), UNSUPPORTED, TOO_LARGE)


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


def test_nothing_here_reaches_a_launch():
    assert {c[0] for c in CASES} == set(BOTH) and len(CASES) > 120
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
    lib = _native.load()
    for fn in BOTH:
        bad, _k = make_args(fn, dict(d=0))
        assert getattr(lib, fn)(*bad) == INVALID
        assert lib.hgd_get_last_error_string() != b""
        good, _k = make_args(fn, dict(EMPTY, n_rows=0))
        assert getattr(lib, fn)(*good) == OK
        assert lib.hgd_get_last_error_string() == b""


# ---- the Python host: what it refuses before it looks for a device ---------------------------
def _csr(n_rows=3, n_cols=2):
    from hypergraph_diffusion_for_recommendation_amd.incidence import CSR
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64)
    return CSR(rowptr, torch.zeros(0, dtype=torch.int32), n_rows, n_cols, split_threshold=0)


def test_spmm_csr_fused_dt_type_errors():
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_csr_fused_dt
    csr, ex = _csr(), _native.RowEpilogue(out_scale=1.0)
    for dt in (torch.float32, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="X16 must be bfloat16"):
            spmm_csr_fused_dt(csr, torch.zeros((2, 8), dtype=dt), ex)
    X16 = torch.zeros((2, 8), dtype=torch.bfloat16)
    for dt in (torch.float32, torch.float16):
        with pytest.raises(TypeError, match="out16 must be bfloat16"):
            spmm_csr_fused_dt(csr, X16, ex, out16=torch.zeros((3, 8), dtype=dt))
    with pytest.raises(TypeError, match="the output must be float32"):
        spmm_csr_fused_dt(csr, X16, ex, out=torch.zeros((3, 8), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="2-D"):
        spmm_csr_fused_dt(csr, torch.zeros(8, dtype=torch.bfloat16), ex)
    # the dtypes are right: the next refusal is the device's, as spmm_csr's
    with pytest.raises(RuntimeError, match="no CPU path"):
        spmm_csr_fused_dt(csr, X16, ex)


@pytest.mark.gpu
def test_spmm_csr_fused_dt_shared_checks_keep_their_prefix(dev):
    """The checks spmm_csr_fused_dt shares with spmm_csr answer in its own words. They come
    after the device's refusal, so the tensors are on the device; each is still rejected before
    anything is launched (the structure's arrays are never read)."""
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_csr_fused_dt
    csr, ex = _csr(), _native.RowEpilogue(out_scale=1.0)
    X16 = torch.zeros((2, 8), dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError) as e:
        spmm_csr_fused_dt(csr, torch.zeros((5, 8), dtype=torch.bfloat16, device=dev), ex)
    assert str(e.value) == "spmm_fused_dt: X16 has 5 rows, structure expects 2"
    with pytest.raises(ValueError) as e:
        spmm_csr_fused_dt(csr, X16, ex, val=torch.zeros(4, device=dev))
    assert str(e.value) == "spmm_fused_dt: val size mismatch"
    with pytest.raises(ValueError) as e:
        spmm_csr_fused_dt(csr, X16, ex, row_scale=torch.zeros(2, device=dev))
    assert str(e.value) == "spmm_fused_dt: row_scale size mismatch"


def test_spmm_csr_still_refuses_a_16_bit_fused_hop():
    """The new path is asked for by name: spmm_csr does not infer it from a tensor's dtype."""
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_csr
    csr, ex = _csr(), _native.RowEpilogue(out_scale=1.0)
    with pytest.raises(TypeError, match="float32-only"):
        spmm_csr(csr, torch.zeros((2, 8), dtype=torch.bfloat16), ex=ex)
    with pytest.raises(TypeError, match="float32-only"):
        spmm_csr(csr, torch.zeros((2, 8)), ex=ex, out_dtype=torch.bfloat16)


@pytest.mark.parametrize("op", ["two_hop_fused", "att_two_hop_fused"])
def test_gather_dtype_type_errors(op):
    from hypergraph_diffusion_for_recommendation_amd import functional as F
    inc = types.SimpleNamespace(n_rows=3, n_cols=3, shape=(3, 3))  # never reached
    X = torch.zeros((3, 8))

    def call(**kw):
        if op == "two_hop_fused":
            return F.two_hop_fused(inc, X, **kw)
        return F.att_two_hop_fused(inc, inc, X, **kw)

    for dt in (torch.float16, torch.float32, torch.float64):
        with pytest.raises(TypeError, match="gather_dtype must be None or torch.bfloat16"):
            call(gather_dtype=dt)
    for dt in (torch.float16, torch.float32):
        with pytest.raises(TypeError, match="x16 must be bfloat16"):
            call(gather_dtype=torch.bfloat16, x16=torch.zeros((3, 8), dtype=dt))
    with pytest.raises(ValueError, match="no copy of X"):
        call(gather_dtype=torch.bfloat16, x16=torch.zeros((3, 16), dtype=torch.bfloat16))
    # x16 / return_x16 never switch the path on by themselves
    with pytest.raises(ValueError, match="go with gather_dtype"):
        call(x16=torch.zeros((3, 8), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="go with gather_dtype"):
        call(return_x16=True)
    # X, the residuals, γ and β stay float32 with the option on, as without it
    with pytest.raises(TypeError, match="float32 only"):
        if op == "two_hop_fused":
            F.two_hop_fused(inc, X.bfloat16(), gather_dtype=torch.bfloat16)
        else:
            F.att_two_hop_fused(inc, inc, X.bfloat16(), gather_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="float32 only"):
        call(gather_dtype=torch.bfloat16, res1=torch.zeros((3, 8), dtype=torch.bfloat16))


def test_encoders_carry_the_attribute():
    from hypergraph_diffusion_for_recommendation_amd import encoders as E
    data = types.SimpleNamespace(n_users=3, n_items=2, norm_adj=None)
    for enc in (E.SelfAwareEncoder(data, 8, 8, 2, 0.2, 0.1, device="cpu", use_self_att=False),
                E.RelationalAwareEncoder(0.2, 0.1, 2, 8),
                E.KHGRecRelationalAwareEncoder(0.2, 0.1, 2, 8)):
        assert enc.gather_dtype is None
        enc.gather_dtype = torch.bfloat16
        del enc.gather_dtype  # a module saved before the attribute existed reads as None
        assert getattr(enc, "gather_dtype", None) is None


def test_bf16_fused_store_layer_norm_rule():
    """Which LayerNorm widths the ops hand to the bf16 fused store: the widths hgd_spmm_fused_dt
    accepts (test_rejection pins d = 68 and 72-with-odd-strides as unsupported), never the fp32
    rule's d % 4 == 0."""
    from hypergraph_diffusion_for_recommendation_amd import functional as F
    for d, ok in ((5, True), (20, True), (64, True), (63, True), (68, False), (100, False),
                  (104, True), (132, False), (252, False), (256, True), (264, False), (320, False)):
        assert F._ln_supported16(d) == ok, d
    assert F._ln_supported(100) and F._ln_supported(68)  # the fp32 store holds them
