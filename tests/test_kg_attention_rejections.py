"""CPU: what the KG-attention entry points answer to a call they reject (argument validation
only: every case returns before the first HIP call, so the pointers are small fake integers and
no device is needed), and the TypeError / ValueError cases the Python surface raises before any
launch. Each C case pins the hgd_status and a message prefixed with the entry's name."""
import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, WORKSPACE = 0, 1, 4
P = 16  # a fake, 16-byte aligned, never dereferenced pointer

SCORES = ["E", "ldE", "n_ent", "W", "R", "ldR", "n_rel", "d", "dr", "h", "t", "grp_perm",
          "rel_off", "rel_enable", "B", "v", "stream"]
SOFTMAX = ["rowptr", "col", "perm", "n_rows", "B", "v", "val", "workspace", "workspace_bytes",
           "stream"]
ORDER = {"hgd_kg_attention_scores": SCORES, "hgd_kg_attention_softmax": SOFTMAX}
VALID = {
    "hgd_kg_attention_scores": dict(E=P, ldE=128, n_ent=97, W=P, R=P, ldR=32, n_rel=5, d=128,
                                    dr=32, h=P, t=P, grp_perm=P, rel_off=P, rel_enable=None,
                                    B=300, v=P, stream=None),
    "hgd_kg_attention_softmax": dict(rowptr=P, col=P, perm=P, n_rows=97, B=300, v=P, val=P,
                                     workspace=P, workspace_bytes=1280, stream=None),
}
S, X = "hgd_kg_attention_scores", "hgd_kg_attention_softmax"

CASES = [
    # null pointers with B > 0
    *[(S, {k: None}, INVALID, "null pointer")
      for k in ("E", "W", "R", "h", "t", "grp_perm", "rel_off", "v")],
    *[(X, {k: None}, INVALID, "null pointer") for k in ("rowptr", "col", "perm", "v", "val")],
    # negative sizes
    (S, dict(B=-1), INVALID, "negative sizes"),
    (S, dict(n_ent=-1), INVALID, "negative sizes"),
    (S, dict(n_rel=-2), INVALID, "negative sizes"),
    (X, dict(B=-1), INVALID, "negative sizes"),
    (X, dict(n_rows=-1), INVALID, "negative sizes"),
    # widths
    (S, dict(d=0), INVALID, "d and dr must be > 0 (got 0, 32)"),
    (S, dict(d=-128), INVALID, "d and dr must be > 0 (got -128, 32)"),
    (S, dict(dr=0), INVALID, "d and dr must be > 0 (got 128, 0)"),
    (S, dict(dr=-1, B=-1), INVALID, "d and dr must be > 0 (got 128, -1)"),
    # leading dimensions below the widths
    (S, dict(ldE=127), INVALID, "ldE must be >= d and ldR >= dr"),
    (S, dict(ldR=31), INVALID, "ldE must be >= d and ldR >= dr"),
    (S, dict(ldE=127, E=None), INVALID, "ldE must be >= d and ldR >= dr"),
    # triples that name nothing
    (S, dict(n_ent=0), INVALID, "triples without entities or relations"),
    (S, dict(n_rel=0), INVALID, "triples without entities or relations"),
    (X, dict(n_rows=0), INVALID, "entries without rows"),
    (S, dict(B=2 ** 31), INVALID, "B out of range"),
    (X, dict(B=2 ** 31), INVALID, "B out of range"),
    # a short workspace (300 scores: 1200 bytes, rounded up to 1280)
    (X, dict(workspace_bytes=1279), WORKSPACE, "workspace 1279 < required 1280"),
    (X, dict(workspace=None), WORKSPACE, "workspace 0 < required 1280"),
    (X, dict(workspace_bytes=0), WORKSPACE, "workspace 0 < required 1280"),
    # B = 0 launches nothing, whatever the pointers
    (S, dict(B=0, E=None, W=None, R=None, h=None, t=None, grp_perm=None, rel_off=None, v=None),
     OK, ""),
    (S, dict(B=0, n_ent=0, n_rel=0), OK, ""),
    (X, dict(B=0, rowptr=None, col=None, perm=None, v=None, val=None, workspace=None,
             workspace_bytes=0), OK, ""),
    (X, dict(B=0, n_rows=0), OK, ""),
]


@pytest.mark.parametrize("fn,over,status,text", CASES,
                         ids=[f"{c[0][17:]}-{'-'.join(c[1])}-{i}" for i, c in enumerate(CASES)])
def test_rejection(fn, over, status, text):
    lib = _native.load()
    args = dict(VALID[fn], **over)
    got = getattr(lib, fn)(*[args[k] for k in ORDER[fn]])
    assert got == status
    assert lib.hgd_get_last_error_string().decode() == (f"{fn}: {text}" if text else "")


def test_workspace_size():
    lib = _native.load()
    assert lib.hgd_kg_attention_softmax_workspace_size(0) == 0
    assert lib.hgd_kg_attention_softmax_workspace_size(-5) == 0
    assert lib.hgd_kg_attention_softmax_workspace_size(300) == 1280
    assert lib.hgd_kg_attention_softmax_workspace_size(8192) == 32768


# ---- the Python surface: raised before anything is launched (no device needed) --------------
def _args(d=8, dr=4, n=10, n_rel=3, B=6):
    return dict(ego_embed=torch.zeros(n, d), h=torch.zeros(B, dtype=torch.int64),
                t=torch.zeros(B, dtype=torch.int64), r=torch.zeros(B, dtype=torch.int64),
                trans_M=torch.zeros(n_rel, d, dr), relation_emb=torch.zeros(n_rel, dr),
                n_entities=n)


@pytest.mark.parametrize("name", ["ego_embed", "trans_M", "relation_emb"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
def test_tables_must_be_float32(name, dtype):
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import kg_attention
    a = _args()
    a[name] = a[name].to(dtype)
    with pytest.raises(TypeError, match=f"{name} must be a float32 tensor"):
        kg_attention(**a)


@pytest.mark.parametrize("name", ["h", "t", "r"])
def test_indices_must_be_int64(name):
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import kg_attention
    a = _args()
    a[name] = a[name].to(torch.int32)
    with pytest.raises(TypeError, match=f"{name} must be an int64 LongTensor"):
        kg_attention(**a)


def test_shape_mismatches():
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import kg_attention
    a = _args()
    with pytest.raises(ValueError, match="differ in length"):
        kg_attention(**dict(a, t=a["t"][:-1]))
    with pytest.raises(ValueError, match="differ in length"):
        kg_attention(**dict(a, r=torch.zeros(7, dtype=torch.int64)))
    with pytest.raises(ValueError, match="must be 1-D"):
        kg_attention(**dict(a, h=a["h"].reshape(2, 3)))
    with pytest.raises(ValueError, match=r"hold 3 / 4 relations"):  # relation counts disagree
        kg_attention(**dict(a, relation_emb=torch.zeros(4, 4)))
    with pytest.raises(ValueError, match="do not match"):  # relation_emb narrower than dr
        kg_attention(**dict(a, relation_emb=torch.zeros(3, 5)))
    with pytest.raises(ValueError, match="do not match"):  # ego_embed width != trans_M's d
        kg_attention(**dict(a, ego_embed=torch.zeros(10, 9)))
    with pytest.raises(ValueError, match="do not match"):  # n_entities != rows of ego_embed
        kg_attention(**dict(a, n_entities=11))
    with pytest.raises(ValueError, match="expected ego_embed"):
        kg_attention(**dict(a, trans_M=torch.zeros(3, 8)))


def test_no_cpu_path():
    """Valid host tensors: there is no CPU fallback, the pattern refuses a host target."""
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import kg_attention
    with pytest.raises(RuntimeError, match="no CPU path"):
        kg_attention(**_args())


def test_conv_checks_before_launch():
    from hypergraph_diffusion_for_recommendation_amd.functional import _check_att
    from types import SimpleNamespace
    att = SimpleNamespace(n_rows=5, n_cols=5, shape=(5, 5))
    inc = SimpleNamespace(n_rows=6, n_cols=3, shape=(6, 3))
    with pytest.raises(TypeError, match="float32 only"):
        _check_att(att, inc, torch.zeros(5, 4, dtype=torch.bfloat16), "att_two_hop")
    with pytest.raises(ValueError, match="att is"):
        _check_att(att, inc, torch.zeros(5, 4), "att_two_hop")
    with pytest.raises(ValueError, match="X "):
        _check_att(att, SimpleNamespace(n_rows=5, n_cols=3, shape=(5, 3)), torch.zeros(6, 4),
                   "att_two_hop")


def test_row_order_opt_out(monkeypatch):
    """A structure marked row_order_ok = False (every KG attention pattern) is never walked in
    row order, not even when HGD_SPMM_ROW_ORDER=1 forces the order wherever it applies."""
    from hypergraph_diffusion_for_recommendation_amd.incidence import CSR, spmm_row_order
    csr = CSR(torch.tensor([0, 1, 2]), torch.zeros(2, dtype=torch.int32), 2, 2, split_threshold=0)
    monkeypatch.setenv("HGD_SPMM_ROW_ORDER", "1")
    assert spmm_row_order(csr, 32)
    csr.row_order_ok = False
    assert not spmm_row_order(csr, 32)
