"""CPU: what hgd_row_epilogue_backward_dt (the fused row epilogue's backward with dZ stored in
bfloat16) answers to a call it rejects, and the errors of its Python host (the ``grad_dtype`` of
functional.two_hop_fused / att_two_hop_fused and of the KG carriers' encoders). Argument
validation only: every case returns before the first HIP call, so the pointers are small fake
integers and no device is needed (the style of tests/test_spmm_fused_dt_rejections.py). Each case
pins the hgd_status and the exact error text."""
import types

import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, BF16 = _native.DT_F32, _native.DT_BF16
P = 16  # a fake, 16-byte aligned, never dereferenced pointer
DT = "hgd_row_epilogue_backward_dt"
FP32 = "hgd_row_epilogue_backward"
DT_CODES = "HGD_DT_F32 or HGD_DT_BF16"
LN_LIMIT = "layer_norm needs d <= 256 (aligned) or <= 64"

ORDER = ["dY", "ldy", "act_out", "ld_act", "stats", "ln_gamma", "n_rows", "d", "act", "slope",
         "layer_norm", "out_scale", "dZ", "dz_dtype", "ldz", "dgamma", "dbeta", "workspace",
         "workspace_bytes", "stream"]
# a call the entry point would launch (LeakyReLU and LayerNorm with dγ / dβ); each case breaks it
WS = 2 * 1024 * 64 * 4  # hgd_row_epilogue_backward_workspace_size(3, 64)
VALID = dict(dY=P, ldy=64, act_out=P, ld_act=64, stats=P, ln_gamma=P, n_rows=3, d=64, act=1,
             slope=0.2, layer_norm=1, out_scale=0.7, dZ=P, dz_dtype=BF16, ldz=64, dgamma=P,
             dbeta=P, workspace=P, workspace_bytes=WS, stream=None)
# the accepted call that needs no device: no rows and nothing to zero
EMPTY = dict(n_rows=0, dY=None, dZ=None, act_out=None, stats=None, dgamma=None, dbeta=None,
             workspace=None, workspace_bytes=0)

CASES = []  # (overrides of VALID, status, error text)


def case(over, status, text, name=DT):
    CASES.append((over, status, f"{name}: {text}" if text else ""))


# the dtype code comes first
case(dict(dz_dtype=2), INVALID, f"unknown dtype code (dz 2): {DT_CODES}")
case(dict(dz_dtype=-1, d=0), INVALID, f"unknown dtype code (dz -1): {DT_CODES}")
case(dict(dz_dtype=7, dZ=None, ldz=0), INVALID, f"unknown dtype code (dz 7): {DT_CODES}")
# HGD_DT_F32 is the fp32 entry point's call, which answers in its own name
case(dict(dz_dtype=F32, d=0), INVALID, "bad sizes", FP32)
case(dict(dz_dtype=F32, ldz=63), INVALID, "ldy/ldz < d", FP32)
case(dict(dz_dtype=F32, dZ=None), INVALID, "null dY/dZ", FP32)
case(dict(dz_dtype=F32, workspace_bytes=WS - 1), WORKSPACE,
     f"workspace {WS - 1} < required {WS}", FP32)
case(dict(EMPTY, dz_dtype=F32), OK, "")
# every check of the fp32 entry point, in the order they run, under the new name
case(dict(d=0), INVALID, "bad sizes")
case(dict(d=-4), INVALID, "bad sizes")
case(dict(n_rows=-1), INVALID, "bad sizes")
case(dict(act=3), INVALID, "bad act")
case(dict(act=-1), INVALID, "bad act")
case(dict(slope=-0.5), INVALID, "activation needs slope >= 0")
case(dict(act=2, slope=-0.5), INVALID, "activation needs slope >= 0")
case(dict(layer_norm=2), INVALID, "layer_norm 0/1")
case(dict(ldy=63), INVALID, "ldy/ldz < d")
case(dict(ldz=63), INVALID, "ldy/ldz < d")  # in bf16 elements, as d
case(dict(ldz=32), INVALID, "ldy/ldz < d")  # 64 columns of bf16 are not 32 floats' worth
case(dict(ldz=0), INVALID, "ldy/ldz < d")
case(dict(ldz=-64), INVALID, "ldy/ldz < d")
case(dict(ldz=63, dZ=None), INVALID, "ldy/ldz < d")
case(dict(dZ=None), INVALID, "null dY/dZ")
case(dict(dY=None), INVALID, "null dY/dZ")
case(dict(dZ=None, act_out=None), INVALID, "null dY/dZ")
case(dict(act_out=None), INVALID, "act_out required")
case(dict(ld_act=63), INVALID, "act_out required")
case(dict(act_out=None, act=0), INVALID, "act_out required")  # LayerNorm alone needs it too
case(dict(act_out=None, layer_norm=0, stats=None), INVALID, "act_out required")
case(dict(stats=None), INVALID, "stats required for layer_norm")
# LayerNorm needs the row in one lane group: 256 columns of 4-column lanes, 64 of one-column
# lanes; a bf16 dZ is on the vector path when it is 8-byte aligned with ldz % 4 == 0
case(dict(d=260, ldy=260, ld_act=260, ldz=260), UNSUPPORTED, LN_LIMIT)
case(dict(d=65, ldy=65, ld_act=65, ldz=65), UNSUPPORTED, LN_LIMIT)
case(dict(d=128, ldy=128, ld_act=128, ldz=128, dZ=P + 2), UNSUPPORTED, LN_LIMIT)
case(dict(d=128, ldy=128, ld_act=128, ldz=128, dZ=P + 4), UNSUPPORTED, LN_LIMIT)
case(dict(d=128, ldy=128, ld_act=128, ldz=130), UNSUPPORTED, LN_LIMIT)
case(dict(d=128, ldy=130, ld_act=128, ldz=128), UNSUPPORTED, LN_LIMIT)
# ... and is not refused for being 8- but not 16-byte aligned: the next check answers
case(dict(d=128, ldy=128, ld_act=128, ldz=132, dZ=P + 8, workspace_bytes=0), WORKSPACE,
     f"workspace 0 < required {2 * 1024 * 128 * 4}")
# the workspace of dγ / dβ: hgd_row_epilogue_backward_workspace_size, unchanged
case(dict(workspace_bytes=WS - 1), WORKSPACE, f"workspace {WS - 1} < required {WS}")
case(dict(workspace=None), WORKSPACE, f"workspace {WS} < required {WS}")
case(dict(workspace_bytes=0, dbeta=None), WORKSPACE, f"workspace 0 < required {WS}")
# accepted without a device: no rows, nothing to zero
case(EMPTY, OK, "")
case(dict(EMPTY, layer_norm=0, act=0), OK, "")
case(dict(EMPTY, ldz=1 << 40), OK, "")


def make_args(over):
    v = dict(VALID, **over)
    return [v[k] for k in ORDER]


def case_id(c):
    return ",".join(f"{k}={x}" for k, x in c[0].items()) or "valid"


def test_symbol_is_exported_and_bound():
    lib = _native.load()
    assert DT in _native._SIGNATURES
    fn = getattr(lib, DT)  # AttributeError if libhgd does not export it
    assert len(fn.argtypes) == len(ORDER)
    # one more argument than the fp32 entry point: the dtype code after dZ
    fp32 = getattr(lib, FP32)
    at = list(fn.argtypes)
    assert at[:13] + at[14:] == list(fp32.argtypes)
    assert lib.hgd_row_epilogue_backward_workspace_size(3, 64) == WS


def test_nothing_here_reaches_a_launch():
    assert len(CASES) > 40
    for over, status, _ in CASES:
        v = dict(VALID, **over)
        assert status != OK or (v["n_rows"] == 0 and v["dgamma"] is None
                                and v["dbeta"] is None), over


@pytest.mark.parametrize("over,status,text", CASES, ids=[case_id(c) for c in CASES])
def test_rejection(over, status, text):
    lib = _native.load()
    got = getattr(lib, DT)(*make_args(over))
    msg = lib.hgd_get_last_error_string().decode()
    print(f"{DT}: status {got}, {msg!r}")
    assert (got, msg) == (status, text)


def test_accepted_call_clears_the_error_text():
    lib = _native.load()
    fn = getattr(lib, DT)
    for dt in (BF16, F32):
        assert fn(*make_args(dict(d=0, dz_dtype=dt))) == INVALID
        assert lib.hgd_get_last_error_string() != b""
        assert fn(*make_args(dict(EMPTY, dz_dtype=dt))) == OK
        assert lib.hgd_get_last_error_string() == b""


# ---- the Python host: what it refuses before it looks for a device ---------------------------
@pytest.mark.parametrize("op", ["two_hop_fused", "att_two_hop_fused"])
def test_grad_dtype_errors(op):
    from hypergraph_diffusion_for_recommendation_amd import functional as F
    inc = types.SimpleNamespace(n_rows=3, n_cols=3, shape=(3, 3))  # never reached
    X = torch.zeros((3, 8))

    def call(**kw):
        if op == "two_hop_fused":
            return F.two_hop_fused(inc, X, **kw)
        return F.att_two_hop_fused(inc, inc, X, **kw)

    # it goes with gather_dtype, and never switches that path on by itself
    with pytest.raises(ValueError) as e:
        call(grad_dtype=torch.bfloat16)
    assert str(e.value) == f"{op}: grad_dtype goes with gather_dtype=torch.bfloat16"
    # bfloat16 or nothing, with and without gather_dtype
    for dt in (torch.float16, torch.float32, torch.float64):
        for kw in ({}, dict(gather_dtype=torch.bfloat16)):
            with pytest.raises(TypeError) as e:
                call(grad_dtype=dt, **kw)
            assert str(e.value) == (f"{op}: grad_dtype must be None or torch.bfloat16, got "
                                    f"{dt}")
    # gather_dtype's own checks still come first
    with pytest.raises(TypeError, match="gather_dtype must be None or torch.bfloat16"):
        call(gather_dtype=torch.float16, grad_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="go with gather_dtype"):
        call(return_x16=True, grad_dtype=torch.bfloat16)


def test_encoders_carry_the_attribute():
    from hypergraph_diffusion_for_recommendation_amd import encoders as E
    data = types.SimpleNamespace(n_users=3, n_items=2, norm_adj=None)
    for enc in (E.SelfAwareEncoder(data, 8, 8, 2, 0.2, 0.1, device="cpu", use_self_att=False),
                E.RelationalAwareEncoder(0.2, 0.1, 2, 8),
                E.KHGRecRelationalAwareEncoder(0.2, 0.1, 2, 8)):
        assert enc.grad_dtype is None and enc.gather_dtype is None
        enc.grad_dtype = torch.bfloat16
        del enc.grad_dtype  # a module saved before the attribute existed reads as None
        assert getattr(enc, "grad_dtype", None) is None
