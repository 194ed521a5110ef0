"""CPU: what kg_loss / kg_loss_rows raise before anything is launched (no device needed), with
their error types, and what the hgd_kg_loss_* entry points answer to a call they reject (argument
validation only: every case returns before the first HIP call, so the pointers are small fake
integers)."""
import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native

REG, BS = 0.01, 8


def _table_args(d=8, dr=4, n=10, n_rel=3, B=6):
    z = torch.zeros(B, dtype=torch.int64)
    return dict(ego_embed=torch.zeros(n, d), h=z, pos_t=z.clone(), neg_t=z.clone(), r=z.clone(),
                trans_M=torch.zeros(n_rel, d, dr), relation_emb=torch.zeros(n_rel, dr),
                reg_kg=REG, batch_size_kg=BS)


def _rows_args(d=8, dr=4, n_rel=3, B=6):
    return dict(h_embed=torch.zeros(B, d), r=torch.zeros(B, dtype=torch.int64),
                pos_t_embed=torch.zeros(B, d), neg_t_embed=torch.zeros(B, d),
                trans_M=torch.zeros(n_rel, d, dr), relation_emb=torch.zeros(n_rel, dr),
                reg_kg=REG, batch_size_kg=BS)


def _call(form, args):
    from hypergraph_diffusion_for_recommendation_amd import kg_loss, kg_loss_rows
    return (kg_loss if form == "table" else kg_loss_rows)(**args)


FLOATS = {"table": ["ego_embed", "trans_M", "relation_emb"],
          "rows": ["h_embed", "pos_t_embed", "neg_t_embed", "trans_M", "relation_emb"]}
INDICES = {"table": ["h", "pos_t", "neg_t", "r"], "rows": ["r"]}
ARGS = {"table": _table_args, "rows": _rows_args}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
@pytest.mark.parametrize("form,name", [(f, n) for f in FLOATS for n in FLOATS[f]])
def test_tables_must_be_float32(form, name, dtype):
    a = ARGS[form]()
    a[name] = a[name].to(dtype)
    with pytest.raises(TypeError, match=f"{name} must be a float32 tensor"):
        _call(form, a)


@pytest.mark.parametrize("form,name", [(f, n) for f in INDICES for n in INDICES[f]])
def test_indices_must_be_int64(form, name):
    a = ARGS[form]()
    a[name] = a[name].to(torch.int32)
    with pytest.raises(TypeError, match=f"{name} must be an int64 LongTensor"):
        _call(form, a)
    a = ARGS[form]()
    a[name] = a[name].reshape(2, 3)
    with pytest.raises(ValueError, match=f"{name} must be 1-D"):
        _call(form, a)


@pytest.mark.parametrize("form", ["table", "rows"])
def test_parameter_shapes(form):
    a = ARGS[form]()
    with pytest.raises(ValueError, match=r"hold 3 / 4 relations"):  # relation counts disagree
        _call(form, dict(a, relation_emb=torch.zeros(4, 4)))
    with pytest.raises(ValueError, match="does not match dr = 4"):
        _call(form, dict(a, relation_emb=torch.zeros(3, 5)))
    with pytest.raises(ValueError, match="expected trans_M"):
        _call(form, dict(a, trans_M=torch.zeros(3, 8)))
    with pytest.raises(ValueError, match="expected trans_M"):
        _call(form, dict(a, relation_emb=torch.zeros(3)))
    with pytest.raises(ValueError, match="relation count"):
        _call(form, dict(a, trans_M=torch.zeros(0, 8, 4), relation_emb=torch.zeros(0, 4)))
    with pytest.raises(ValueError, match="batch_size_kg must be > 0"):
        _call(form, dict(a, batch_size_kg=0))


def test_table_form_shapes():
    a = _table_args()
    with pytest.raises(ValueError, match="does not match d = 8"):
        _call("table", dict(a, ego_embed=torch.zeros(10, 9)))
    with pytest.raises(ValueError, match="does not match d = 8"):
        _call("table", dict(a, ego_embed=torch.zeros(10, 2, 4)))
    for name in ("pos_t", "neg_t", "r"):
        with pytest.raises(ValueError, match="differ in length"):
            _call("table", dict(a, **{name: a[name][:-1]}))
    e = torch.zeros(0, dtype=torch.int64)
    with pytest.raises(ValueError, match="empty batch"):
        _call("table", dict(a, h=e, pos_t=e, neg_t=e, r=e))


def test_rows_form_shapes():
    a = _rows_args()
    for name in ("h_embed", "pos_t_embed", "neg_t_embed"):
        with pytest.raises(ValueError, match=f"{name} .* does not match 6 triples"):
            _call("rows", dict(a, **{name: torch.zeros(5, 8)}))  # a length mismatch
        with pytest.raises(ValueError, match=f"{name} .* does not match 6 triples"):
            _call("rows", dict(a, **{name: torch.zeros(6, 9)}))
        with pytest.raises(ValueError, match=f"{name} .* does not match 6 triples"):
            _call("rows", dict(a, **{name: torch.zeros(6 * 8)}))
    with pytest.raises(ValueError, match="empty batch"):
        _call("rows", dict(a, r=a["r"][:0], **{k: a[k][:0] for k in (
            "h_embed", "pos_t_embed", "neg_t_embed")}))


@pytest.mark.parametrize("form", ["table", "rows"])
def test_no_cpu_path(form):
    """Valid host tensors: there is no CPU fallback."""
    with pytest.raises(RuntimeError, match="no CPU path"):
        _call(form, ARGS[form]())


def test_pattern_must_match_the_call():
    """A pattern of another batch (or of other sizes) is refused before any launch."""
    from types import SimpleNamespace
    a = _table_args()
    for over in (dict(B=5), dict(n_entities=11), dict(n_relations=4)):
        pat = SimpleNamespace(**dict(dict(B=6, n_entities=10, n_relations=3,
                                          h32=torch.zeros(6, dtype=torch.int32)), **over))
        with pytest.raises(ValueError, match="the pattern is of"):
            _call("table", dict(a, pattern=pat))


# ---- the C entry points ---------------------------------------------------------------------
OK, INVALID, WORKSPACE = 0, 1, 4
P = 16  # a fake, never dereferenced pointer
ROWS = ["xh", "ldh", "ih", "xp", "ldp", "ip", "xn", "ldn", "in"]
COMMON = ROWS + ["W", "R", "ldR", "n_rel", "d", "dr", "grp_perm", "rel_off", "B", "reg_kg",
                 "batch_size_kg"]
ORDER = {
    "hgd_kg_loss_forward": COMMON + ["proj", "coef", "norms", "loss", "workspace",
                                     "workspace_bytes", "stream"],
    "hgd_kg_loss_backward": COMMON + ["proj", "coef", "norms", "grad", "G", "dW", "dR",
                                      "workspace", "workspace_bytes", "stream"],
}
_COMMON = dict(xh=P, ldh=128, ih=P, xp=P, ldp=128, ip=P, xn=P, ldn=128, W=P, R=P, ldR=32,
               n_rel=5, d=128, dr=32, grp_perm=P, rel_off=P, B=300, reg_kg=0.01,
               batch_size_kg=8192, proj=P, coef=P, norms=P, workspace=P,
               workspace_bytes=1 << 30, stream=None)
_COMMON["in"] = P
VALID = {"hgd_kg_loss_forward": dict(_COMMON, loss=P),
         "hgd_kg_loss_backward": dict(_COMMON, grad=P, G=P, dW=P, dR=P)}
F, Bk = "hgd_kg_loss_forward", "hgd_kg_loss_backward"

CASES = [
    *[(fn, {k: None}, INVALID, "null pointer")
      for fn in (F, Bk) for k in ("xh", "xp", "xn", "W", "R", "grp_perm", "rel_off", "proj",
                                  "coef", "norms")],
    (F, dict(loss=None), INVALID, "null pointer"),
    (Bk, dict(grad=None), INVALID, "null pointer"),
    *[(fn, dict(B=0), INVALID, "B must be > 0 (the mean over no triples is undefined)")
      for fn in (F, Bk)],
    (F, dict(B=-3), INVALID, "B must be > 0 (the mean over no triples is undefined)"),
    (F, dict(B=2 ** 31), INVALID, "B out of range"),
    (F, dict(d=0), INVALID, "d and dr must be > 0 (got 0, 32)"),
    (Bk, dict(dr=-1), INVALID, "d and dr must be > 0 (got 128, -1)"),
    (F, dict(d=1 << 20, ldh=1 << 20, ldp=1 << 20, ldn=1 << 20), INVALID, "d * dr out of range"),
    (F, dict(n_rel=0), INVALID, "n_rel must be in [1, 65535] (got 0)"),
    (Bk, dict(n_rel=65536), INVALID, "n_rel must be in [1, 65535] (got 65536)"),
    (F, dict(batch_size_kg=0), INVALID, "batch_size_kg must be > 0"),
    *[(F, {k: 127}, INVALID, "the rows' leading dimensions must be >= d and ldR >= dr")
      for k in ("ldh", "ldp", "ldn")],
    (Bk, dict(ldR=31), INVALID, "the rows' leading dimensions must be >= d and ldR >= dr"),
    (Bk, dict(dW=None), INVALID, "dW and dR go together"),
    (Bk, dict(dR=None), INVALID, "dW and dR go together"),
    # 300 triples of 5 relations: 15 tiles; 15 · 8 floats of partial sums = 480 → 512 bytes
    (F, dict(workspace_bytes=511), WORKSPACE, "workspace 511 < required 512"),
    (F, dict(workspace=None), WORKSPACE, "workspace 0 < required 512"),
    # + 15 tiles of (128 + 1) · 32 floats = 247680 → 247808 bytes
    (Bk, dict(G=None, workspace_bytes=1000), WORKSPACE, "workspace 1000 < required 248320"),
]


@pytest.mark.parametrize("fn,over,status,text", CASES,
                         ids=[f"{c[0][12:]}-{'-'.join(c[1])}-{i}" for i, c in enumerate(CASES)])
def test_rejection(fn, over, status, text):
    lib = _native.load()
    args = dict(VALID[fn], **over)
    got = getattr(lib, fn)(*[args[k] for k in ORDER[fn]])
    assert got == status
    assert lib.hgd_get_last_error_string().decode() == f"{fn}: {text}"


def test_workspace_size():
    lib = _native.load()
    assert lib.hgd_kg_loss_workspace_size(0, 5, 128, 32) == 0
    assert lib.hgd_kg_loss_workspace_size(300, 0, 128, 32) == 0
    assert lib.hgd_kg_loss_workspace_size(300, 5, 128, 32) == 512 + 247808
    # the KHGRec shape: 256 + 40 tiles
    assert lib.hgd_kg_loss_workspace_size(8192, 40, 128, 32) == 9472 + 296 * 129 * 32 * 4
