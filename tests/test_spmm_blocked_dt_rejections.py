"""CPU: what the source-blocked hop over 16-bit tables (hgd_spmm_blocked_dt) answers to a call
it rejects, what its workspace query and its size rule return, and what profiling.impl_bytes
counts for it. Argument validation only: every case returns before the first HIP call, so the
pointers are small fake integers and no device is needed (the style of
tests/test_spmm_rejections.py). Each case pins the hgd_status and the exact error text."""
import pytest

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
F32, BF16 = _native.DT_F32, _native.DT_BF16
P = 16  # a fake, 16-byte aligned, never dereferenced pointer
FN = "hgd_spmm_blocked_dt"
DT_CODES = "HGD_DT_F32 or HGD_DT_BF16"

ORDER = ["blk_start", "blk_col", "blk_val", "row_scale", "n_rows", "n_src_rows", "row_begin",
         "row_end", "X", "x_dtype", "ldx", "Y", "y_dtype", "ldy", "d", "epilogue", "slope",
         "n_blocks", "workspace", "workspace_bytes", "stream"]
# 3 rows × 64 columns × 4 B of fp32 partials = 768 B: a call that would launch
NEED = 768
VALID = dict(blk_start=P, blk_col=P, blk_val=None, row_scale=None, n_rows=3, n_src_rows=2,
             row_begin=0, row_end=3, X=P, x_dtype=BF16, ldx=64, Y=P, y_dtype=BF16, ldy=64, d=64,
             epilogue=0, slope=0.0, n_blocks=2, workspace=P, workspace_bytes=NEED, stream=None)
EMPTY = dict(blk_start=None, blk_col=None, X=None, Y=None, workspace=None, workspace_bytes=0,
             row_begin=0, row_end=0)  # all-null call over an empty range
# More rows than the widest grid: at d = 64 a bf16 hop's group is 8 lanes, 32 rows per workgroup,
# so 2^37 rows are 2^32 workgroups. The launcher refuses that grid after it has taken the
# workspace and before it launches anything: the answer of an ACCEPTED workspace without a device.
HUGE = dict(n_rows=1 << 37, row_end=1 << 37)
TOO_LARGE = "grid too large"

CASES = []  # (overrides of VALID, status, error text, the entry point the message names)


def case(over, status, text, name=FN):
    CASES.append((over, status, f"{name}: {text}" if text else ""))


# dtype codes come first
case(dict(x_dtype=2), INVALID, f"unknown dtype code (x 2, y 1): {DT_CODES}")
case(dict(y_dtype=-1, d=0), INVALID, f"unknown dtype code (x 1, y -1): {DT_CODES}")
case(dict(x_dtype=2, n_blocks=0), INVALID, f"unknown dtype code (x 2, y 1): {DT_CODES}")
# the blocks, before the shared checks
case(dict(n_blocks=0), INVALID, "blocks must be 1..64")
case(dict(n_blocks=65), INVALID, "blocks must be 1..64")
case(dict(n_blocks=-1), INVALID, "blocks must be 1..64")
case(dict(blk_start=None), INVALID, "null blk_start")
case(dict(n_blocks=0, blk_start=None, d=0), INVALID, "blocks must be 1..64")
case(dict(blk_start=None, d=0), INVALID, "null blk_start")
case(dict(EMPTY, n_blocks=65), INVALID, "blocks must be 1..64")
# the shared size / range / ld checks, for every mixed pair
for codes in (dict(), dict(y_dtype=F32), dict(x_dtype=F32)):
    case(dict(codes, d=0), INVALID, "d must be > 0 (got 0)")
    case(dict(codes, d=-4), INVALID, "d must be > 0 (got -4)")
    case(dict(codes, n_src_rows=-1), INVALID, "negative sizes")
    case(dict(codes, n_rows=-3, row_end=0), INVALID, "negative sizes")
    case(dict(codes, row_end=4), INVALID, "row range [0,4) outside [0,3)")
    case(dict(codes, row_begin=-1), INVALID, "row range [-1,3) outside [0,3)")
    case(dict(codes, row_begin=2, row_end=1), INVALID, "row range [2,1) outside [0,3)")
    case(dict(codes, ldx=63), INVALID, "ldx/ldy must be >= d")
    case(dict(codes, ldy=63), INVALID, "ldx/ldy must be >= d")
    case(dict(codes, epilogue=3), INVALID, "bad epilogue 3")
    case(dict(codes, Y=None), INVALID, "null rowptr/Y")
    case(dict(codes, X=None), INVALID, "null X")
    case(dict(codes, **EMPTY), OK, "")
    case(dict(codes, **dict(EMPTY, row_begin=2, row_end=2)), OK, "")
# the workspace of a bf16 output in more than one block: the launcher's message shape
case(dict(workspace_bytes=NEED - 1), WORKSPACE, f"workspace {NEED - 1} < required {NEED}")
case(dict(workspace_bytes=0, workspace=None), WORKSPACE, f"workspace 0 < required {NEED}")
case(dict(workspace=None), WORKSPACE, f"workspace {NEED} < required {NEED}")
case(dict(x_dtype=F32, workspace_bytes=NEED - 1), WORKSPACE,
     f"workspace {NEED - 1} < required {NEED}")
case(dict(n_blocks=5, workspace_bytes=NEED - 1), WORKSPACE,
     f"workspace {NEED - 1} < required {NEED}")
case(dict(workspace_bytes=0, Y=None), INVALID, "null rowptr/Y")  # the shared checks win
# d = 7 (the scalar path): 3 × 7 × 4 = 84 B, rounded up to 256
case(dict(d=7, workspace_bytes=255), WORKSPACE, "workspace 255 < required 256")
# ... and a zero workspace is accepted for an fp32 output and for one block (see HUGE)
case(dict(HUGE, workspace=None, workspace_bytes=0), WORKSPACE,
     f"workspace 0 < required {(1 << 37) * 64 * 4}")
case(dict(HUGE, y_dtype=F32, workspace=None, workspace_bytes=0), UNSUPPORTED, TOO_LARGE)
case(dict(HUGE, n_blocks=1, workspace=None, workspace_bytes=0), UNSUPPORTED, TOO_LARGE)
case(dict(HUGE, n_blocks=1, x_dtype=F32, workspace=None, workspace_bytes=0), UNSUPPORTED,
     TOO_LARGE)
# f32 → f32 is hgd_spmm_blocked's call, and says so
BOTH = dict(x_dtype=F32, y_dtype=F32)
case(dict(BOTH, d=0), INVALID, "d must be > 0 (got 0)", name="hgd_spmm_blocked")
case(dict(BOTH, n_blocks=0), INVALID, "blocks must be 1..64", name="hgd_spmm_blocked")
case(dict(BOTH, blk_start=None), INVALID, "null blk_start", name="hgd_spmm_blocked")
case(dict(BOTH, epilogue=3), INVALID, "bad epilogue 3", name="hgd_spmm_blocked")
case(dict(BOTH, **EMPTY), OK, "")


def case_id(c):
    return ",".join(f"{k}={x}" for k, x in c[0].items()) or "valid"


def test_nothing_here_reaches_a_launch():
    assert len(CASES) > 60
    for over, status, _ in CASES:
        v = dict(VALID, **over)
        assert status != OK or v["row_begin"] == v["row_end"], over


@pytest.mark.parametrize("over,status,text", CASES, ids=[case_id(c) for c in CASES])
def test_rejection(over, status, text):
    lib = _native.load()
    v = dict(VALID, **over)
    got = lib.hgd_spmm_blocked_dt(*[v[k] for k in ORDER])
    msg = lib.hgd_get_last_error_string().decode()
    print(f"{FN}: status {got}, {msg!r}")
    assert (got, msg) == (status, text)


def test_accepted_call_clears_the_error_text():
    lib = _native.load()
    bad = dict(VALID, d=0)
    assert lib.hgd_spmm_blocked_dt(*[bad[k] for k in ORDER]) == INVALID
    assert lib.hgd_get_last_error_string() != b""
    good = dict(VALID, **dict(EMPTY, n_rows=0))
    assert lib.hgd_spmm_blocked_dt(*[good[k] for k in ORDER]) == OK
    assert lib.hgd_get_last_error_string() == b""


def test_workspace_size():
    """The fp32 partials of a bf16 output at the hop's full width, rounded up to 256 B; nothing
    for an fp32 output (it holds its own partial) or for one block (the plain hop)."""
    f = _native.load().hgd_spmm_blocked_dt_workspace_size
    for n_blocks in (2, 3, 64):
        assert f(3, 64, BF16, n_blocks) == 768
        assert f(613, 64, BF16, n_blocks) == 613 * 64 * 4
        assert f(613, 7, BF16, n_blocks) == (613 * 7 * 4 + 255) // 256 * 256
        assert f(1_000_000, 256, BF16, n_blocks) == 1_000_000 * 256 * 4
        assert f(1 << 33, 64, BF16, n_blocks) == (1 << 33) * 256  # past 2^32 bytes
        assert f(613, 64, F32, n_blocks) == 0
    for y in (F32, BF16):
        assert f(613, 64, y, 1) == 0 and f(613, 64, y, 0) == 0
        assert f(0, 64, y, 2) == 0 and f(613, 0, y, 2) == 0


def test_size_rule_for_f32_is_the_fp32_rule():
    """hgd_spmm_blocks_for_dt(n, d, HGD_DT_F32) == hgd_spmm_blocks_for(n, d) over the shapes of
    tests/test_spmm_blocks_policy.py."""
    lib = _native.load()
    f, g = lib.hgd_spmm_blocks_for_dt, lib.hgd_spmm_blocks_for
    mib640 = 640 << 20
    shapes = [(0, 64), (10_000_000, 0), (10_000_000, 64), (10_000_000, 128), (10_000_000, 512),
              (10_000_000, 256), (10_000_000, 1024), (10_000_000, 32), (2_000_000, 256),
              (1_000_000, 256), (100_000_000, 64), (1_000_000, 64), (5_000_000, 32),
              (2_500_000, 32), ((1 << 29) // 256 - 1, 64), ((1 << 29) // 256, 64),
              ((1 << 30) // 256 - 1, 64), ((1 << 30) // 256, 64)]
    shapes += [(int(x * mib640) // 256, 64) for x in (4.5, 5.5, 6.4, 6.6)]
    answers = set()
    for n, d in shapes:
        assert f(n, d, F32) == g(n, d), (n, d)
        answers.add(g(n, d))
    assert answers >= {0, 2, 4, 6, 7, 8, 16}  # the shapes do exercise the rule


def test_spmm_blocks_takes_the_table_dtype(monkeypatch):
    """incidence.spmm_blocks: the fp32 answers unchanged with the dtype spelled out, the
    environment override reaching a bfloat16 hop, the structure rules before either."""
    import torch

    from hypergraph_diffusion_for_recommendation_amd.incidence import CSR, spmm_blocks

    def csr(n_rows, n_cols, nnz=10, ascending=True):
        rowptr = torch.zeros(n_rows + 1, dtype=torch.int64)
        rowptr[-1] = nnz
        s = CSR(rowptr, torch.zeros(nnz, dtype=torch.int32), n_rows, n_cols, split_threshold=0)
        s.cols_ascending = ascending
        return s

    lib = _native.load()
    monkeypatch.delenv("HGD_SPMM_BLOCKS", raising=False)
    big = csr(1_000_000, 10_000_000)
    assert spmm_blocks(big, 64, torch.float32) == spmm_blocks(big, 64) == 4
    assert spmm_blocks(big, 64, torch.bfloat16) == lib.hgd_spmm_blocks_for_dt(10_000_000, 64, BF16)
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "3")
    small = csr(100, 1000)
    assert spmm_blocks(small, 8, torch.bfloat16) == 3
    assert spmm_blocks(csr(100, 1000, ascending=False), 8, torch.bfloat16) == 0
    assert spmm_blocks(csr(100, 1000, nnz=0), 8, torch.bfloat16) == 0
    small.mask = torch.ones(10, dtype=torch.uint8)  # an edge-dropped view: the masked kernel
    assert spmm_blocks(small, 8, torch.bfloat16) == 0 and spmm_blocks(small, 8) == 0
    monkeypatch.setenv("HGD_SPMM_BLOCKS", "1")
    assert spmm_blocks(csr(100, 1000), 8, torch.bfloat16) == 0
    with pytest.raises(TypeError):
        spmm_blocks(csr(100, 1000), 8, torch.float16)


def test_blocked_16_bit_implementation_bytes():
    """profiling.impl_bytes of a blocked 16-bit hop against the traffic written out: the index
    and weight streams and the gathered rows at the table's element size, the [R × (P+1)] int64
    block starts, the row scale once per block, and
      * fp32 Y: P writes and P−1 reads of the 4-byte Y row (the partial lives in Y);
      * bf16 Y: P−1 writes and P−1 reads of the 4-byte scratch row, then ONE 2-byte Y row."""
    from hypergraph_diffusion_for_recommendation_amd import profiling
    nnz, R, d = 1000, 100, 64
    for P_ in (2, 4, 5):
        for hv in (False, True):
            for hs in (False, True):
                for xb in (2, 4):
                    stream = nnz * (4 + (4 if hv else 0) + xb * d) + R * (P_ + 1) * 8
                    scale = R * 4 * P_ if hs else 0
                    f32_y = R * 4 * d * (P_ + (P_ - 1))
                    bf16_y = R * 4 * d * 2 * (P_ - 1) + R * 2 * d
                    assert profiling.impl_bytes(nnz, R, d, hv, hs, P_, x_bytes=xb,
                                                y_bytes=4) == stream + scale + f32_y
                    assert profiling.impl_bytes(nnz, R, d, hv, hs, P_, x_bytes=xb,
                                                y_bytes=2) == stream + scale + bf16_y
    # one block is the plain hop, whatever the types
    for yb in (2, 4):
        assert (profiling.impl_bytes(nnz, R, d, True, True, 1, x_bytes=2, y_bytes=yb)
                == profiling.impl_bytes(nnz, R, d, True, True, 0, x_bytes=2, y_bytes=yb))
