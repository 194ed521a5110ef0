"""CPU: the float64 references and the sentinel check of tests/_gemm_ref64.py, before any GPU
test relies on them — ``rows_ref64`` / ``tn_ref64`` against plain torch.float64 matmuls written
out independently, the workspace formula, the sentinel check firing on one changed padding
element, and the share of elements the ReLU sign filter skips at the GPU tests' shapes."""
import numpy as np
import pytest
import torch

from oracle import hgd_oracle as O
from tests import _gemm_ref64 as G


def _t(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def _flat_b(f, ldw=None):
    """What launch_rows fills in: the weight in a padded flat buffer and its two strides."""
    W = f["W"]
    ldw = ldw or W.shape[1] + 16
    buf = np.full((W.shape[0], ldw), 3.0e38, dtype=np.float32)
    buf[:, :W.shape[1]] = W
    f["B"] = buf.reshape(-1)
    f["bsk"], f["bsn"] = (1, ldw) if f["orient"] == "fwd" else (ldw, 1)
    return f


@pytest.mark.parametrize("orient", ["fwd", "bwd"])
def test_rows_ref64_plain_bias_relu(orient):
    f = _flat_b(G.make_rows_case(1, 37, 48, 80, orient))
    ref = G.rows_ref64(f)
    Bm = _t(f["W"]).T if orient == "fwd" else _t(f["W"])
    z = _t(f["A"]) @ Bm + _t(f["bias"])
    assert torch.allclose(torch.from_numpy(ref["Y"]), z.clamp_min(0), rtol=1e-13, atol=1e-13)
    mag = _t(f["A"]).abs() @ Bm.abs() + _t(f["bias"]).abs()
    assert torch.allclose(torch.from_numpy(ref["mag"]), mag, rtol=1e-13, atol=0)


def test_rows_ref64_mask_dropout_accumulate():
    """relu_mask + accumulate + both dropouts: the header's order (input dropout, mask, product,
    bias, ReLU, output dropout, accumulate)."""
    f = _flat_b(G.make_rows_case(2, 33, 32, 48, "bwd",
                                 opts=("relu_mask", "accumulate", "drop", "a_drop")))
    ref = G.rows_ref64(f)
    ka = _t(O.dropout_keep_mask(f["a_drop_seed"], 33 * 32, 0.5).reshape(33, 32))
    kd = _t(O.dropout_keep_mask(f["drop_seed"], 33 * 48, 0.75).reshape(33, 48))
    A = _t(f["A"]) * ka * 2.0 * _t(f["relu_mask"] > 0)
    y = (A @ _t(f["W"]) + _t(f["bias"])).clamp_min(0) * kd * float(np.float32(1 / 0.75))
    assert torch.allclose(torch.from_numpy(ref["Y"]), y + _t(f["Y_in"]), rtol=1e-13, atol=1e-13)
    assert 0.2 < ka.mean() < 0.8 and 0.5 < kd.mean() < 0.95  # the draws are not degenerate


def test_rows_ref64_binarize_row_inv_counts_scale_residual():
    f = _flat_b(G.make_rows_case(3, 21, 64, 32, "fwd", relu=False,
                                 opts=("binarize_row_inv", "b_row_count", "b_scale", "res")))
    ref = G.rows_ref64(f)
    A = _t(f["A"] > 0)
    B = _t(f["W"]).T / _t(np.maximum(f["b_row_count"], 1))[:, None] * 1.25
    inv = 1.0 / A.sum(1).clamp_min(1.0)
    y = (A @ B) * inv[:, None] + _t(f["bias"])
    assert torch.allclose(torch.from_numpy(ref["Y"]), y, rtol=1e-13, atol=1e-13)
    assert torch.allclose(torch.from_numpy(ref["Y2"]), y + _t(f["res"]), rtol=1e-13, atol=1e-13)
    assert torch.allclose(torch.from_numpy(ref["row_inv"]), inv, rtol=1e-15, atol=0)
    assert ref["row_inv"][2] == 1.0  # the row without a positive entry


def test_tn_ref64_against_torch():
    f = G.make_tn_case(4, 131, 48, 80, opts=("relu_mask", "colsum", "b_row_scale", "c_scale",
                                             "b_drop"))
    ref = G.tn_ref64(f)
    kb = _t(O.dropout_keep_mask(f["b_drop_seed"], 131 * 80, 0.75).reshape(131, 80))
    A = _t(f["A"]) * _t(f["relu_mask"] > 0)
    B = _t(f["B"]) * kb * float(np.float32(1 / 0.75)) * _t(f["b_row_scale"])[:, None]
    assert torch.allclose(torch.from_numpy(ref["C"]), A.T @ B * 1.25, rtol=1e-13, atol=1e-13)
    assert torch.allclose(torch.from_numpy(ref["colsum"]), A.sum(0) * 1.25, rtol=1e-13, atol=1e-13)
    g = G.make_tn_case(5, 70, 16, 16, opts=("binarize", "colsum"))
    ref = G.tn_ref64(g)
    assert np.array_equal(ref["colsum"], (g["A"] > 0).sum(0))  # binarize_a counts nonzeros
    assert torch.allclose(torch.from_numpy(ref["C"]), _t(g["A"] > 0).T @ _t(g["B"]),
                          rtol=1e-13, atol=1e-13)


def test_workspace_formula():
    # 1,031 rows in 64-row slices: 17 slices; 17·48·80·4 = 261,120 B (a multiple of 256) plus
    # 17·48·4 = 3,264 → 3,328 B with colsum_A
    assert G.tn_workspace_bytes(1031, 48, 80, False, 64) == 261_120
    assert G.tn_workspace_bytes(1031, 48, 80, True, 64) == 261_120 + 3_328
    assert G.tn_workspace_bytes(1, 16, 16, True, 4096) == 1024 + 256
    assert G.tn_workspace_bytes(0, 16, 16, True, 64) == 0


def test_sentinel_check_fires_on_one_padding_element():
    rows, width, ld, start = 5, 16, 20, 44
    buf = np.full(start + rows * ld + 44, G.SENTINEL, dtype=np.int32)
    idx = start + np.arange(rows)[:, None] * ld + np.arange(width)[None, :]
    buf[idx.reshape(-1)] = 7
    G.check_outside(buf, start, rows, width, ld)  # everything inside may change
    for where in (start + 2 * ld + width, start - 1, start + rows * ld, len(buf) - 1):
        bad = buf.copy()
        bad[where] = 0
        with pytest.raises(AssertionError, match="outside"):
            G.check_outside(bad, start, rows, width, ld, what="Y")


def test_relu_sign_filter_skips_far_less_than_one_percent():
    """The GPU tests compare only elements with |z| > 1e-5·Σ|terms| in float64 and assert the
    skipped share < 1 %; with the standard-normal operands of make_rows_case it is ~1e-5."""
    worst = 0.0
    for rows, K, N in ((257, 16, 272), (257, 128, 144), (1031, 64, 48), (17, 32, 32)):
        for opts in ((), ("drop",), ("a_drop", "res"), ("binarize_row_inv",), ("b_row_count",)):
            f = _flat_b(G.make_rows_case(rows + K + N, rows, K, N, "fwd", opts=opts))
            ref = G.rows_ref64(f)
            worst = max(worst, 1.0 - G.sign_ok(f, ref).mean())
    assert worst < 1e-3, worst


def test_exact_units_counts_the_roundings():
    f = G.make_rows_case(0, 4, 32, 16)
    assert G.exact_units(f) == 34
    f = G.make_rows_case(0, 4, 128, 16, opts=("binarize_row_inv", "drop", "res"))
    assert G.exact_units(f) == 128 + 2 + 2 + 1 + 1
    assert G.exact_units(f) * G.U24 < 1e-5  # tighter than the project bound at every K <= 128


# ---------------------------------------------------------------------------------------------
# Host-only checks of the library (they return before any HIP call: no GPU needed)


def _tn_desc(rows, M, N, colsum):
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    d = nat.GemmTnDesc()
    d.A, d.lda, d.B, d.ldb, d.rows, d.M, d.N, d.C = 16, M, 16, N, rows, M, N, 16
    d.colsum_A = 16 if colsum else None
    return d


@pytest.mark.parametrize("form", [{}, {"X3_SPLITK": 0}, {"X3_SPLITK": 1}, {"GEMM_EXACT": 1},
                                  {"X3P_QUEUE": 1}])
@pytest.mark.parametrize("slice_rows", [64, 192, 4096])
def test_workspace_size_follows_splitk_rows(form, slice_rows):
    """hgd_gemm_tn_workspace_size under HGD_TUNE_SPLITK_ROWS = r is what include/hgd.h implies —
    ⌈rows / r⌉ slices of M·N floats (+ M with colsum_A), each part 256-byte aligned — for every
    kernel form, single products and groups with an empty member."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    with G.tuning(lib, SPLITK_ROWS=slice_rows, **form):
        for M, N in ((16, 16), (48, 80), (64, 64), (128, 128), (32, 272)):
            for rows in (1, 64, 65, 4099, 70_001):
                for colsum in (False, True):
                    arr = (nat.GemmTnDesc * 1)(_tn_desc(rows, M, N, colsum))
                    assert lib.hgd_gemm_tn_workspace_size(arr, 1) == G.tn_workspace_bytes(
                        rows, M, N, colsum, slice_rows), (M, N, rows, colsum)
        arr = (nat.GemmTnDesc * 2)(_tn_desc(70_001, 64, 64, True), _tn_desc(33, 64, 64, True))
        assert lib.hgd_gemm_tn_workspace_size(arr, 2) == (
            G.tn_workspace_bytes(70_001, 64, 64, True, slice_rows)
            + G.tn_workspace_bytes(33, 64, 64, True, slice_rows))
        arr = (nat.GemmTnDesc * 2)(_tn_desc(0, 64, 64, True), _tn_desc(65, 64, 64, False))
        assert lib.hgd_gemm_tn_workspace_size(arr, 2) == G.tn_workspace_bytes(
            65, 64, 64, False, slice_rows)
    # and the keys are back at their defaults
    arr = (nat.GemmTnDesc * 1)(_tn_desc(70_001, 128, 128, True))
    before = lib.hgd_gemm_tn_workspace_size(arr, 1)
    with G.tuning(lib, SPLITK_ROWS=64):
        assert lib.hgd_gemm_tn_workspace_size(arr, 1) != before
    assert lib.hgd_gemm_tn_workspace_size(arr, 1) == before


def test_gemm_tn_rejects_a_short_workspace_before_any_launch():
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    arr = (nat.GemmTnDesc * 1)(_tn_desc(1031, 48, 80, True))
    need = lib.hgd_gemm_tn_workspace_size(arr, 1)
    assert need > 0
    assert lib.hgd_gemm_tn(arr, 1, 256, need - 1, None) == 4  # HGD_ERR_WORKSPACE
    assert b"workspace" in lib.hgd_get_last_error_string()


@pytest.mark.parametrize("form", [{}, {"X3S_TILES": 1}, {"X3_COLS": 64}, {"X3_COLS": 128},
                                  {"GEMM_EXACT": 1}])
def test_gemm_rows_group_rejects_mixed_epilogues(form):
    """accumulate on one member, a residual on the other: HGD_ERR_INVALID_ARG under every kernel
    form (the check sits in front of the dispatch), also when the other member is empty."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()

    def desc(rows, **kw):
        d = nat.GemmRowsDesc()
        d.A, d.lda, d.B, d.bsk, d.bsn, d.Y, d.ldy = 16, 64, 16, 1, 64, 16, 64
        d.rows, d.K, d.N = rows, 64, 64
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    with G.tuning(lib, **form):
        for rows in ((65, 65), (65, 0)):
            arr = (nat.GemmRowsDesc * 2)(desc(rows[0], accumulate=1),
                                         desc(rows[1], res=16, ldres=64, Y2=16, ldy2=64))
            assert lib.hgd_gemm_rows(arr, 2, None) == 1
            assert b"same epilogue" in lib.hgd_get_last_error_string()
