"""CPU: what view_attention / view_attention_stacked / layers.Attention raise before anything is
launched (no device needed), what a CPU-tensor call returns (the reference's expression), and
what the hgd_view_attention_* entry points answer to a call they reject (argument validation
only: every case returns before the first HIP call, so the pointers are small fake integers)."""
import pytest
import torch
import torch.nn.functional as F

from hypergraph_diffusion_for_recommendation_amd import _native


def _args(N=6, d=16):
    return dict(z0=torch.zeros(N, d), z1=torch.zeros(N, d), weight1=torch.zeros(d, d),
                bias1=torch.zeros(d), weight2=torch.zeros(d, d))


def _call(a):
    from hypergraph_diffusion_for_recommendation_amd import view_attention
    return view_attention(**a)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
@pytest.mark.parametrize("name", ["z0", "z1", "weight1", "bias1", "weight2"])
def test_tensors_must_be_float32(name, dtype):
    a = _args()
    a[name] = a[name].to(dtype)
    with pytest.raises(TypeError, match=f"{name} must be a float32 tensor"):
        _call(a)


def test_stacked_must_be_float32():
    from hypergraph_diffusion_for_recommendation_amd import view_attention_stacked
    a = _args()
    with pytest.raises(TypeError, match="z must be a float32 tensor"):
        view_attention_stacked(torch.zeros(6, 2, 16, dtype=torch.bfloat16), a["weight1"],
                               a["bias1"], a["weight2"])
    with pytest.raises(TypeError, match="weight2 must be a float32 tensor"):
        view_attention_stacked(torch.zeros(6, 2, 16), a["weight1"], a["bias1"], None)


def test_shapes():
    from hypergraph_diffusion_for_recommendation_amd import view_attention_stacked
    a = _args()
    with pytest.raises(ValueError, match=r"z0 and z1 must be \[N, d\]"):
        _call(dict(a, z0=torch.zeros(6, 2, 16)))
    with pytest.raises(ValueError, match=r"z0 and z1 must be \[N, d\]"):
        _call(dict(a, z1=torch.zeros(96)))
    with pytest.raises(ValueError, match=r"z0 \(6, 16\) and z1 \(5, 16\) differ"):
        _call(dict(a, z1=torch.zeros(5, 16)))
    with pytest.raises(ValueError, match=r"z0 \(6, 16\) and z1 \(6, 32\) differ"):
        _call(dict(a, z1=torch.zeros(6, 32)))
    with pytest.raises(ValueError, match="weight1 .* does not match d = 16"):
        _call(dict(a, weight1=torch.zeros(16, 20)))
    with pytest.raises(ValueError, match="weight1 .* does not match d = 16"):
        _call(dict(a, weight1=torch.zeros(16)))
    with pytest.raises(ValueError, match="weight1 .*hidden_size must equal in_size = 16 .*"
                                         "beta \\* z broadcast"):
        _call(dict(a, weight1=torch.zeros(32, 16), bias1=torch.zeros(32),
                   weight2=torch.zeros(32, 32)))
    with pytest.raises(ValueError, match="bias1 .* does not match d = 16"):
        _call(dict(a, bias1=torch.zeros(17)))
    with pytest.raises(ValueError, match="weight2 .* does not match d = 16"):
        _call(dict(a, weight2=torch.zeros(16, 17)))
    with pytest.raises(ValueError, match=r"z must be \[N, 2, d\]"):
        view_attention_stacked(torch.zeros(6, 3, 16), a["weight1"], a["bias1"], a["weight2"])
    with pytest.raises(ValueError, match=r"z must be \[N, 2, d\]"):
        view_attention_stacked(torch.zeros(6, 16), a["weight1"], a["bias1"], a["weight2"])


@pytest.mark.parametrize("name", ["z1", "weight1", "bias1", "weight2"])
def test_devices_must_match(name):
    a = _args()
    a[name] = a[name].to("meta")
    with pytest.raises(RuntimeError, match=f"{name} is on meta, z0 on cpu"):
        _call(a)


def test_hidden_size_must_equal_in_size():
    from hypergraph_diffusion_for_recommendation_amd.layers import Attention
    with pytest.raises(ValueError, match="hidden_size = 128 must equal in_size = 64.*broadcasts"):
        Attention(64)
    with pytest.raises(ValueError, match="hidden_size = 32 must equal in_size = 64"):
        Attention(64, hidden_size=32)
    m = Attention(128)
    assert sorted(m.state_dict()) == ["project.0.bias", "project.0.weight", "project.2.weight"]


@pytest.mark.parametrize("d", [16, 20, 128])
def test_cpu_tensors_run_the_reference_expression(d):
    from hypergraph_diffusion_for_recommendation_amd import (view_attention,
                                                             view_attention_supported)
    from hypergraph_diffusion_for_recommendation_amd.layers import Attention
    g = torch.Generator().manual_seed(d)
    z = torch.randn(9, 2, d, generator=g)
    m = Attention(d, d)
    W1, b1, W2 = m.weights()
    assert not view_attention_supported(z[:, 0], z[:, 1], W1, b1, W2)
    assert not view_attention_supported(z)
    with torch.no_grad():
        beta = torch.softmax(F.linear(torch.tanh(F.linear(z, W1, b1)), W2), dim=1)
        want = (beta * z).sum(1)
        out, got_beta = view_attention(z[:, 0], z[:, 1], W1, b1, W2, return_beta=True)
        assert torch.equal(out, want) and torch.equal(got_beta, beta)
        assert torch.equal(view_attention(z[:, 0], z[:, 1], W1, b1, W2), want)
        fused, mb = m(z)
        assert torch.equal(fused, want) and torch.equal(mb, beta)
        m.need_beta = False
        assert m(z)[1] is None
    # the fallback is differentiable into the views and the parameters; beta is not
    z0, z1 = (z[:, v].clone().requires_grad_(True) for v in (0, 1))
    out, b = view_attention(z0, z1, W1, b1, W2, return_beta=True)
    assert not b.requires_grad
    out.sum().backward()
    assert z0.grad is not None and z1.grad is not None and W1.grad is not None


# ---- the C entry points ---------------------------------------------------------------------
OK, INVALID = 0, 1
P = 16   # a fake, never dereferenced, 16-byte aligned pointer
Q = 20   # a misaligned one
COMMON = ["z0", "ld0", "z1", "ld1", "n_rows", "d", "W1", "b1", "W2"]
ORDER = {
    "hgd_view_attention_forward": COMMON + ["out", "ldo", "beta0", "ldb", "stream"],
    "hgd_view_attention_backward": COMMON + ["beta0", "ldb", "g", "ldg", "dz0", "lddz0", "dz1",
                                             "lddz1", "dW1", "db1", "dW2", "workspace",
                                             "workspace_bytes", "stream"],
}
_COMMON = dict(z0=P, ld0=128, z1=P, ld1=256, n_rows=300, d=128, W1=P, b1=P, W2=P, beta0=P,
               ldb=128, stream=None)
Fw, Bk = "hgd_view_attention_forward", "hgd_view_attention_backward"
VALID = {Fw: dict(_COMMON, out=P, ldo=128),
         Bk: dict(_COMMON, g=P, ldg=128, dz0=P, lddz0=128, dz1=P, lddz1=256, dW1=P, db1=P,
                  dW2=P, workspace=P, workspace_bytes=1 << 30)}
NOT_FUSED = "is not a fused width (a multiple of 16 in [16, 128])"

CASES = [
    *[(fn, dict(d=d), f"d = {d} {NOT_FUSED}") for fn in (Fw, Bk) for d in (0, 8, 20, 144, -16)],
    *[(fn, {k: None}, "null pointer") for fn in (Fw, Bk)
      for k in ("z0", "z1", "W1", "b1", "W2")],
    (Fw, dict(out=None), "null pointer"),
    (Bk, dict(beta0=None), "null pointer"),
    (Bk, dict(g=None), "null pointer"),
    *[(fn, {k: 127}, "the views' leading dimensions must be >= d") for fn in (Fw, Bk)
      for k in ("ld0", "ld1")],
    *[(fn, {k: Q}, "the views' rows must be 16-byte aligned") for fn in (Fw, Bk)
      for k in ("z0", "z1")],
    *[(fn, {k: 130}, "the views' rows must be 16-byte aligned") for fn in (Fw, Bk)
      for k in ("ld0", "ld1")],
    (Fw, dict(n_rows=-1), "n_rows out of range"),
    (Fw, dict(ldo=64), "ldo / ldb must be >= d"),
    (Fw, dict(ldb=64), "ldo / ldb must be >= d"),
    (Fw, dict(out=Q), "the rows of out / beta0 must be 16-byte aligned"),
    (Fw, dict(beta0=Q), "the rows of out / beta0 must be 16-byte aligned"),
    (Fw, dict(ldo=129), "the rows of out / beta0 must be 16-byte aligned"),
    (Bk, dict(ldb=64), "ldb / ldg must be >= d"),
    (Bk, dict(ldg=64), "ldb / ldg must be >= d"),
    (Bk, dict(g=Q), "the rows of beta0 / g must be 16-byte aligned"),
    (Bk, dict(ldg=129), "the rows of beta0 / g must be 16-byte aligned"),
    (Bk, dict(dz0=None), "dz0 and dz1 go together"),
    (Bk, dict(dz1=None), "dz0 and dz1 go together"),
    (Bk, dict(lddz1=64), "lddz0 / lddz1 must be >= d"),
    (Bk, dict(dz0=Q), "the rows of dz0 / dz1 must be 16-byte aligned"),
    (Bk, dict(lddz1=258), "the rows of dz0 / dz1 must be 16-byte aligned"),
    (Bk, dict(dW1=None), "dW1, db1 and dW2 go together"),
    (Bk, dict(db1=None), "dW1, db1 and dW2 go together"),
    (Bk, dict(dW2=None), "dW1, db1 and dW2 go together"),
    (Bk, dict(dz0=None, dz1=None, dW1=None, db1=None, dW2=None),
     "nothing to compute (no dz, no parameter gradients)"),
    (Bk, dict(workspace=None), "null or misaligned workspace"),
    (Bk, dict(workspace=Q), "null or misaligned workspace"),
]


@pytest.mark.parametrize("fn,over,text", CASES,
                         ids=[f"{c[0][19:]}-{'-'.join(c[1])}-{i}" for i, c in enumerate(CASES)])
def test_rejection(fn, over, text):
    lib = _native.load()
    args = dict(VALID[fn], **over)
    got = getattr(lib, fn)(*[args[k] for k in ORDER[fn]])
    assert got == INVALID
    assert lib.hgd_get_last_error_string().decode() == f"{fn}: {text}"


def test_workspace_too_small():
    lib = _native.load()
    need = lib.hgd_view_attention_workspace_size(300, 128, 128, 256)
    assert need >= 4 * 300 * 128 * 4
    args = dict(VALID[Bk], workspace_bytes=need - 1)
    assert getattr(lib, Bk)(*[args[k] for k in ORDER[Bk]]) == INVALID
    assert lib.hgd_get_last_error_string().decode() == \
        f"{Bk}: workspace {need - 1} < required {need}"


def test_no_rows_is_accepted_without_a_launch():
    lib = _native.load()
    for fn in (Fw, Bk):
        args = dict(VALID[fn], n_rows=0)
        assert getattr(lib, fn)(*[args[k] for k in ORDER[fn]]) == OK


def test_workspace_size():
    from hypergraph_diffusion_for_recommendation_amd.view_attention import ROW_BLOCK
    lib = _native.load()
    assert lib.hgd_view_attention_row_block() == ROW_BLOCK
    size = lib.hgd_view_attention_workspace_size
    assert size(0, 128, 128, 128) == 0 and size(-5, 128, 128, 128) == 0
    assert size(300, 20, 20, 20) == 0 and size(300, 144, 144, 144) == 0
    assert size(300, 128, 64, 128) == 0
    for d in (16, 48, 128):
        sizes = [size(n, d, d, 2 * d) for n in (1, 31, 32, 33, 300, 1000, 4096, 100000, 1000000)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (d, sizes)
        assert sizes[-1] >= 4 * 1000000 * d * 4
