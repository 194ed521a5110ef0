"""CPU: the 16-bit hop's ABI (hgd_spmm_dt / hgd_spmm_masked_dt) — exported and bound symbols, the
dtype codes, argument validation that returns before any launch, and the byte model of
profiling.hop_bytes / impl_bytes with element sizes. No device work."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hgd_spmm_dt", "hgd_spmm_masked_dt")


def _header_defines():
    text = open(os.path.join(ROOT, "include", "hgd.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(HGD_DT_\w+)\s+(\d+)\s*$", text,
                                             flags=re.M)}


def test_library_exports_and_binds_the_dt_symbols():
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    raw = ctypes.CDLL(nat.LIB_PATH)
    lib = nat.load()
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in nat.symbols()
        assert getattr(lib, name).restype is ctypes.c_int32


def test_dtype_codes_match_the_header():
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    defs = _header_defines()
    assert defs == {"HGD_DT_F32": nat.DT_F32, "HGD_DT_BF16": nat.DT_BF16}
    assert nat.DT_F32 != nat.DT_BF16


def _call(lib, masked, *, x_dtype, y_dtype, d=8, n_rows=4, row_begin=0, row_end=4, ldx=8, ldy=8):
    """One call with fake (never dereferenced) device addresses: every case below must return in
    the argument checks, before any launch."""
    p = 4096
    if masked:
        return lib.hgd_spmm_masked_dt(p, p, None, p, 0.5, None, n_rows, 4, row_begin, row_end, p,
                                      x_dtype, ldx, p, y_dtype, ldy, d, 0, 0.0, None, None, 0,
                                      None)
    return lib.hgd_spmm_dt(p, p, None, None, n_rows, 4, row_begin, row_end, p, x_dtype, ldx, p,
                           y_dtype, ldy, d, 0, 0.0, None, None, 0, None)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pair", ["bf16_bf16", "bf16_f32", "f32_bf16", "f32_f32"])
def test_dt_argument_validation_returns_before_any_launch(masked, pair):
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    code = {"bf16": nat.DT_BF16, "f32": nat.DT_F32}
    xd, yd = (code[s] for s in pair.split("_"))
    name = NEW[1] if masked else NEW[0]

    def err():
        return lib.hgd_get_last_error_string().decode()

    bad = [dict(x_dtype=7, y_dtype=yd), dict(x_dtype=xd, y_dtype=-1), dict(x_dtype=2, y_dtype=2)]
    for kw in bad:  # an unknown dtype code
        assert _call(lib, masked, **kw) == 1, kw  # HGD_ERR_INVALID_ARG
        assert name in err() and "dtype" in err()
    for d in (0, -3):
        assert _call(lib, masked, x_dtype=xd, y_dtype=yd, d=d) == 1
        assert "d must be > 0" in err()
    for rb, re_ in ((0, 5), (-1, 2), (3, 2)):  # outside [0, n_rows) or reversed
        assert _call(lib, masked, x_dtype=xd, y_dtype=yd, row_begin=rb, row_end=re_) == 1
        assert "row range" in err()
    assert _call(lib, masked, x_dtype=xd, y_dtype=yd, ldx=7) == 1
    assert "ldx" in err()
    assert _call(lib, masked, x_dtype=xd, y_dtype=yd, ldy=7) == 1
    assert "ldy" in err()
    # an empty row range is a valid no-op and clears the error text
    assert _call(lib, masked, x_dtype=xd, y_dtype=yd, row_begin=2, row_end=2) == 0
    assert err() == ""


def _parent_hop_bytes(nnz, rows, d, weighted=False):
    return nnz * (4 + (4 if weighted else 0) + 4 * d) + rows * (4 * d + 4) + (rows + 1) * 4


def _parent_impl_bytes(nnz, rows, d, has_val, has_scale, blocks=0):
    if blocks > 1:
        return (nnz * (4 + (4 if has_val else 0) + 4 * d)
                + rows * (4 * d * (2 * blocks - 1) + (4 * blocks if has_scale else 0))
                + rows * (blocks + 1) * 8)
    return (nnz * (4 + (4 if has_val else 0) + 4 * d)
            + rows * (4 * d + (4 if has_scale else 0)) + (rows + 1) * 8)


@pytest.mark.parametrize("shape", [(99_999_492, 1_000_000, 64), (2500, 173, 7)])
def test_byte_model_defaults_are_the_fp32_values(shape):
    """hop_bytes / impl_bytes without element sizes: exactly the fp32 figures they returned before
    the 16-bit hop existed (restated here from that formula, and as literals for the bench hop)."""
    from hypergraph_diffusion_for_recommendation_amd import profiling as P
    nnz, rows, d = shape
    for weighted in (False, True):
        assert P.hop_bytes(nnz, rows, d, weighted) == _parent_hop_bytes(nnz, rows, d, weighted)
        assert P.hop_bytes(nnz, rows, d, weighted, x_bytes=4, y_bytes=4) == \
            _parent_hop_bytes(nnz, rows, d, weighted)
    for hv in (False, True):
        for hs in (False, True):
            for blocks in (0, 1, 4):
                assert P.impl_bytes(nnz, rows, d, hv, hs, blocks) == \
                    _parent_impl_bytes(nnz, rows, d, hv, hs, blocks)
    if d == 64:
        assert P.hop_bytes(nnz, rows, d) == 26_263_867_924
        assert P.impl_bytes(nnz, rows, d, True, True) == 26_667_865_896
    else:
        assert P.hop_bytes(nnz, rows, d) == 2500 * 32 + 173 * 32 + 174 * 4


def test_byte_model_with_two_byte_elements():
    """B_hop(ex, ey) = nnz·(4 + ex·d) + R·(ey·d + 4) + (R+1)·4."""
    from hypergraph_diffusion_for_recommendation_amd import profiling as P

    def b_hop(nnz, rows, d, ex, ey):
        return nnz * (4 + ex * d) + rows * (ey * d + 4) + (rows + 1) * 4

    items = (99_999_492, 1_000_000, 64)   # the bench graph's hop into items
    users = (99_999_492, 10_000_000, 64)  # and into users
    assert P.hop_bytes(*items, x_bytes=2, y_bytes=2) == b_hop(*items, 2, 2) == 13_335_932_948
    assert P.hop_bytes(*users, x_bytes=2, y_bytes=2) == b_hop(*users, 2, 2)
    assert P.hop_bytes(*items, x_bytes=2, y_bytes=4) == b_hop(*items, 2, 4)
    assert P.hop_bytes(*items, x_bytes=4, y_bytes=2) == b_hop(*items, 4, 2)
    for nnz, rows, d in (items, (2500, 173, 7)):
        assert P.hop_bytes(nnz, rows, d, x_bytes=2, y_bytes=2) == b_hop(nnz, rows, d, 2, 2)
        assert P.hop_bytes(nnz, rows, d, True, x_bytes=2, y_bytes=2) == \
            b_hop(nnz, rows, d, 2, 2) + 4 * nnz
        # as implemented: int64 rowptr, optional weights and scales
        assert P.impl_bytes(nnz, rows, d, True, True, x_bytes=2, y_bytes=2) == \
            nnz * (8 + 2 * d) + rows * (2 * d + 4) + (rows + 1) * 8
        assert P.impl_bytes(nnz, rows, d, False, False, x_bytes=2, y_bytes=4) == \
            nnz * (4 + 2 * d) + rows * (4 * d) + (rows + 1) * 8
    # the forward+backward of one hgconv2 at d = 64: two hops into items, two into users
    fp32 = 2 * (P.hop_bytes(*items) + P.hop_bytes(*users))
    bf16 = 2 * (P.hop_bytes(*items, x_bytes=2, y_bytes=2)
                + P.hop_bytes(*users, x_bytes=2, y_bytes=2))
    assert round(fp32 / 1e9, 1) == 109.8 and round(bf16 / 1e9, 1) == 55.8
