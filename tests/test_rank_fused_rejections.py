"""CPU: what hgd_rank_topk answers to a call it rejects (argument validation only: every case
returns before the first HIP call, so the pointers are small fake integers), the workspace size as
a function of its arguments, and what evaluation.rank_users(fused=True) raises before anything is
launched."""
import itertools

import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 3, 4
P = 16  # a fake, never dereferenced pointer
ORDER = ["user_emb", "ldu", "item_emb", "ldi", "n_items", "d", "users", "n_rows", "rated_rowptr",
         "rated_cols", "mask_value", "k", "n_segments", "out_ids", "out_scores", "workspace",
         "workspace_bytes", "stream"]
VALID = dict(user_emb=P, ldu=64, item_emb=P, ldi=64, n_items=1000, d=64, users=P, n_rows=100,
             rated_rowptr=P, rated_cols=P, mask_value=-10e8, k=40, n_segments=0, out_ids=P,
             out_scores=P, workspace=P, workspace_bytes=1 << 40, stream=None)

CASES = [
    *[({name: None}, INVALID) for name in ("user_emb", "item_emb", "out_ids", "out_scores")],
    (dict(d=0), INVALID),
    (dict(d=-1), INVALID),
    (dict(k=0), INVALID),
    (dict(k=-2), INVALID),
    (dict(k=41, n_items=40), INVALID),
    (dict(ldu=63), INVALID),
    (dict(ldi=63), INVALID),
    (dict(n_segments=-1), INVALID),
    (dict(n_items=2 ** 31), INVALID),
    (dict(n_items=-1), INVALID),
    (dict(n_rows=-1), INVALID),
    (dict(k=65), UNSUPPORTED),
    (dict(d=257, ldu=257, ldi=257), UNSUPPORTED),
    (dict(workspace_bytes=0), WORKSPACE),
    (dict(workspace=None), WORKSPACE),
    (dict(n_rows=0), OK),
    (dict(n_rows=0, workspace=None, workspace_bytes=0, out_ids=None, user_emb=None), OK),
]


def _call(lib, **over):
    args = dict(VALID, **over)
    return lib.hgd_rank_topk(*[args[name] for name in ORDER])


@pytest.mark.parametrize("over,status", CASES,
                         ids=[f"{'-'.join(c[0])}-{i}" for i, c in enumerate(CASES)])
def test_rejection(over, status):
    lib = _native.load()
    assert _call(lib, **over) == status
    text = lib.hgd_get_last_error_string().decode()
    assert (text == "") == (status == OK)
    assert status == OK or text.startswith("hgd_rank_topk: ")


def test_limits_are_named():
    lib = _native.load()
    assert _call(lib, k=65) == UNSUPPORTED
    assert "HGD_RANK_MAX_K = 64" in lib.hgd_get_last_error_string().decode()
    assert _call(lib, d=300, ldu=300, ldi=300) == UNSUPPORTED
    assert "HGD_RANK_MAX_D = 256" in lib.hgd_get_last_error_string().decode()


def test_workspace_one_byte_short():
    lib = _native.load()
    need = lib.hgd_rank_topk_workspace_size(100, 1000, 40, 0)
    assert need > 0
    assert _call(lib, workspace_bytes=need - 1) == WORKSPACE
    assert f"{need} needed" in lib.hgd_get_last_error_string().decode()


def test_geometry():
    import ctypes
    lib = _native.load()
    tu, ti, slots = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib.hgd_rank_topk_geometry(ctypes.byref(tu), ctypes.byref(ti), ctypes.byref(slots))
    assert ti.value >= 64 and tu.value % 16 == 0 and slots.value >= ti.value + 64
    lib.hgd_rank_topk_geometry(None, None, None)  # every output is optional


ROWS = (1, 63, 64, 65, 192, 256, 1000, 16384, 65536)
ITEMS = (64, 65, 512, 513, 1000, 38048, 1_000_000)
KS = (1, 20, 40, 64)
SEGS = (0, 1, 2, 3, 7, 64, 1000)


def test_workspace_size_is_a_monotone_pure_function():
    lib = _native.load()
    size = lib.hgd_rank_topk_workspace_size
    table = {a: size(*a) for a in itertools.product(ROWS, ITEMS, KS, SEGS)}
    for a, v in table.items():
        assert v > 0 and size(*a) == v  # the same arguments, the same answer
    for (i, grid) in enumerate((ROWS, ITEMS, KS)):
        for a, v in table.items():
            j = grid.index(a[i])
            if j + 1 < len(grid):
                b = a[:i] + (grid[j + 1],) + a[i + 1:]
                assert table[b] >= v, (a, b)
    explicit = [s for s in SEGS if s]  # 0 is "by shape", not the smallest count
    for a, v in table.items():
        if a[3] and a[3] != explicit[-1]:
            b = a[:3] + (explicit[explicit.index(a[3]) + 1],)
            assert table[b] >= v, (a, b)
    # exact: k seeds per row (256-byte aligned) + (score, id) per row, segment and k
    assert size(100, 1000, 40, 3) == 16128 + 100 * 3 * 40 * 8
    assert size(100, 1000, 40, 1000) == 16128 + 100 * 16 * 40 * 8  # clamped to the 16 tiles
    assert size(0, 1000, 40, 0) == 0 and size(100, 1000, 40, -1) == 0


# ---- the Python errors ------------------------------------------------------------------------
def _tables(n=10, m=100, d=8, dtype=torch.float32):
    return torch.zeros(n, d, dtype=dtype), torch.zeros(m, d, dtype=dtype)


def test_python_rejects_host_and_non_fp32_tensors():
    from hypergraph_diffusion_for_recommendation_amd.evaluation import rank_users
    ue, ie = _tables()
    users = torch.arange(4)
    with pytest.raises(TypeError, match="user_emb must be a 2-D float32 device tensor"):
        rank_users(ue, ie, users, None, 5, fused=True)
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        bad, _ = _tables(dtype=dtype)
        with pytest.raises(TypeError, match="user_emb must be a 2-D float32 device tensor"):
            rank_users(bad, ie, users, None, 5, fused=True)
        with pytest.raises(TypeError, match="item_emb must be a 2-D float32 device tensor"):
            rank_users(ue, ie.to(dtype), users, None, 5, fused=True)
    with pytest.raises(TypeError, match="item_emb must be a 2-D float32 device tensor"):
        rank_users(ue, ie[0], users, None, 5, fused=True)


def test_python_names_the_limits():
    from hypergraph_diffusion_for_recommendation_amd import evaluation as ev
    users = torch.arange(4)
    ue, ie = _tables(d=8)
    with pytest.raises(ValueError, match="k = 65 exceeds HGD_RANK_MAX_K = 64"):
        ev.rank_users(ue, ie, users, None, 65, fused=True)
    ue, ie = _tables(d=257)
    with pytest.raises(ValueError, match="d = 257 exceeds HGD_RANK_MAX_D = 256"):
        ev.rank_users(ue, ie, users, None, 5, fused=True)
    ue, ie = _tables(m=3)
    with pytest.raises(ValueError, match="k = 5 of 3 items"):
        ev.rank_users(ue, ie, users, None, 5, fused=True)
    ue, ie = _tables()
    with pytest.raises(ValueError, match="segments must be >= 0"):
        ev.rank_users(ue, ie, users, None, 5, fused=True, segments=-1)
    with pytest.raises(ValueError, match="widths 8 and 9 differ"):
        ev.rank_users(ue, torch.zeros(100, 9), users, None, 5, fused=True)
    assert (ev.RANK_MAX_K, ev.RANK_MAX_D) == (64, 256)
