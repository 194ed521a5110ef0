"""CPU: what cf_loss raises before anything is launched (no device needed), what a CPU-tensor
call returns (the reference's expression, within the suite's bound of the float64 restatement),
and what the hgd_cf_loss_* entry points answer to a call they reject (argument validation only:
every case returns before the first HIP call, so the pointers are small fake integers)."""
import pytest
import torch

from hypergraph_diffusion_for_recommendation_amd import _native
from tests import _cf_loss_ref64 as R
from tests._util import RTOL, assert_close


def _args(B=5, d=16, n_users=7, n_items=9):
    return dict(user_emb=torch.zeros(n_users, d), item_cf=torch.zeros(n_items, d),
                item_kg=torch.zeros(n_items, d), uid=torch.zeros(B, dtype=torch.int64),
                pid=torch.zeros(B, dtype=torch.int64), nid=torch.zeros(B, dtype=torch.int64),
                reg=0.01, batch_size=2048, W1=torch.zeros(d, d), b1=torch.zeros(d),
                W2=torch.zeros(d, d))


def _call(a):
    from hypergraph_diffusion_for_recommendation_amd import cf_loss
    return cf_loss(**a)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
@pytest.mark.parametrize("name", ["user_emb", "item_cf", "item_kg", "W1", "b1", "W2"])
def test_tensors_must_be_float32(name, dtype):
    a = _args()
    a[name] = a[name].to(dtype)
    with pytest.raises(TypeError, match=f"{name} must be a float32 tensor"):
        _call(a)


@pytest.mark.parametrize("name", ["uid", "pid", "nid"])
def test_ids_must_be_int64(name):
    a = _args()
    a[name] = a[name].to(torch.int32)
    with pytest.raises(TypeError, match=f"{name} must be an int64 LongTensor"):
        _call(a)


def test_shapes():
    a = _args()
    with pytest.raises(ValueError, match=r"user_emb must be \[n, d\]"):
        _call(dict(a, user_emb=torch.zeros(7, 2, 16)))
    with pytest.raises(ValueError, match=r"item_kg must be \[n, d\]"):
        _call(dict(a, item_kg=torch.zeros(144)))
    with pytest.raises(ValueError, match=r"item_cf \(9, 16\) and item_kg \(8, 16\) differ"):
        _call(dict(a, item_kg=torch.zeros(8, 16)))
    with pytest.raises(ValueError, match=r"item_cf \(9, 32\) does not match d = 16"):
        _call(dict(a, item_cf=torch.zeros(9, 32), item_kg=torch.zeros(9, 32)))
    with pytest.raises(ValueError, match="W1 .* does not match d = 16"):
        _call(dict(a, W1=torch.zeros(16, 20)))
    with pytest.raises(ValueError, match="b1 .* does not match d = 16"):
        _call(dict(a, b1=torch.zeros(17)))
    with pytest.raises(ValueError, match="W2 .* does not match d = 16"):
        _call(dict(a, W2=torch.zeros(16)))
    with pytest.raises(ValueError, match="pid must be 1-D"):
        _call(dict(a, pid=torch.zeros(5, 1, dtype=torch.int64)))
    with pytest.raises(ValueError, match=r"uid, pid, nid differ in length \(5, 5, 4\)"):
        _call(dict(a, nid=torch.zeros(4, dtype=torch.int64)))


def test_empty_batch_and_batch_size():
    a = _args(B=0)
    with pytest.raises(ValueError, match="an empty batch has no loss"):
        _call(a)
    for bs in (0, -3):
        with pytest.raises(ValueError, match="batch_size must be > 0"):
            _call(dict(_args(), batch_size=bs))


@pytest.mark.parametrize("missing", [("W1",), ("b1",), ("W2",), ("W1", "b1"), ("b1", "W2")])
def test_parameters_go_together(missing):
    a = _args()
    for k in missing:
        a[k] = None
    with pytest.raises(ValueError, match="W1, b1 and W2 go together"):
        _call(a)


def test_attention_argument():
    from hypergraph_diffusion_for_recommendation_amd import cf_loss
    from hypergraph_diffusion_for_recommendation_amd.layers import Attention
    a = _args()
    m = Attention(16, 16)
    with pytest.raises(ValueError, match="give attention= or W1, b1, W2, not both"):
        cf_loss(**a, attention=m)
    for k in ("W1", "b1", "W2"):
        a.pop(k)
    inp = R.inputs(5, 16)
    with torch.no_grad():
        got = cf_loss(inp["users"], inp["z0"], inp["z1"], inp["uid"], inp["pid"], inp["nid"],
                      0.01, 2048, attention=m)
        want = cf_loss(inp["users"], inp["z0"], inp["z1"], inp["uid"], inp["pid"], inp["nid"],
                       0.01, 2048, *m.weights())
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["item_cf", "item_kg", "W1", "b1", "W2"])
def test_devices_must_match(name):
    a = _args()
    a[name] = a[name].to("meta")
    with pytest.raises(RuntimeError, match=f"{name} is on meta, user_emb on cpu"):
        _call(a)


@pytest.mark.parametrize("attention", [True, False])
def test_cpu_tensors_run_the_reference_expression(attention):
    from hypergraph_diffusion_for_recommendation_amd import cf_loss, cf_loss_supported
    B, d, reg, bs = 17, 32, 0.01, 2048
    inp = R.inputs(B, d)
    ref, mag = R.reference(inp, reg, bs, attention)
    names = ("users", "z0", "z1") + (("W1", "b1", "W2") if attention else ())
    leaves = [inp[k].clone().requires_grad_(True) for k in names]
    assert not cf_loss_supported(*leaves)
    loss = cf_loss(*leaves[:3], inp["uid"], inp["pid"], inp["nid"], reg, bs, *leaves[3:])
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    got = dict(loss=loss.detach(), **{k: x.grad for k, x in zip(R.GRADS, leaves)})
    for k, v in got.items():
        err = (v.double() - ref[k]).abs()
        print(f"cpu attention={attention} {k}: max err / mag = "
              f"{float((err / (mag[k] + 1e-30)).max()):.3e}")
        assert_close(v.numpy(), ref[k].numpy(), mag[k].numpy(), RTOL, k)


# ---- the C entry points ---------------------------------------------------------------------
OK, INVALID, WORKSPACE = 0, 1, 4
P = 16   # a fake, never dereferenced, 16-byte aligned pointer
Q = 20   # a misaligned one
COMMON = ["U", "ldu", "uid", "n_users", "Z0", "ld0", "Z1", "ld1", "pid", "nid", "n_items",
          "batch", "d", "W1", "b1", "W2", "reg", "batch_size"]
Fw, Bk = "hgd_cf_loss_forward", "hgd_cf_loss_backward"
ORDER = {
    Fw: COMMON + ["beta0", "ldb", "coef", "norms", "loss", "workspace", "workspace_bytes",
                  "stream"],
    Bk: COMMON + ["beta0", "ldb", "coef", "norms", "grad", "dA", "ldda", "dZ0", "lddz0", "dZ1",
                  "lddz1", "dW1", "db1", "dW2", "workspace", "workspace_bytes", "stream"],
}
_COMMON = dict(U=P, ldu=128, uid=P, n_users=40, Z0=P, ld0=128, Z1=P, ld1=256, pid=P, nid=P,
               n_items=300, batch=64, d=128, W1=P, b1=P, W2=P, reg=0.01, batch_size=2048,
               beta0=P, ldb=128, coef=P, norms=P, workspace=P, workspace_bytes=1 << 30,
               stream=None)
VALID = {Fw: dict(_COMMON, loss=P),
         Bk: dict(_COMMON, grad=P, dA=P, ldda=128, dZ0=P, lddz0=128, dZ1=P, lddz1=256, dW1=P,
                  db1=P, dW2=P)}
MEAN = dict(W1=None, b1=None, W2=None, beta0=None, dW1=None, db1=None, dW2=None)
NOT_FUSED = "is not a fused width (a multiple of 16 in [16, 128])"
NOT_MEAN = "is not a mean-mode width (a multiple of 4 in [4, 256])"
BOTH = (Fw, Bk)

CASES = [
    *[(fn, dict(d=d), f"d = {d} {NOT_FUSED}") for fn in BOTH for d in (0, 8, 20, 144, -16)],
    *[(fn, dict(MEAN, d=d), f"d = {d} {NOT_MEAN}") for fn in BOTH for d in (0, 2, 18, 260)],
    *[(fn, {k: None}, "W1, b1 and W2 go together (all NULL = the mean of the views)")
      for fn in BOTH for k in ("W1", "b1", "W2")],
    *[(fn, {k: None}, "null pointer") for fn in BOTH
      for k in ("U", "uid", "Z0", "Z1", "pid", "nid", "coef", "norms")],
    (Fw, dict(loss=None), "null pointer"),
    (Bk, dict(grad=None), "null pointer"),
    (Bk, dict(beta0=None), "null pointer"),
    *[(fn, {k: 127}, "the rows' leading dimensions must be >= d") for fn in BOTH
      for k in ("ldu", "ld0", "ld1")],
    *[(fn, {k: Q}, "the rows of U / Z0 / Z1 must be 16-byte aligned") for fn in BOTH
      for k in ("U", "Z0", "Z1")],
    *[(fn, {k: 130}, "the rows of U / Z0 / Z1 must be 16-byte aligned") for fn in BOTH
      for k in ("ldu", "ld0", "ld1")],
    *[(fn, dict(batch=-1), "batch out of range") for fn in BOTH],
    *[(fn, dict(batch_size=0), "batch_size must be > 0") for fn in BOTH],
    *[(fn, dict(n_items=0), "n_users / n_items out of range") for fn in BOTH],
    (Fw, dict(MEAN, beta0=P), "beta0 belongs to the attention mode"),
    *[(fn, dict(ldb=64), "ldb must be >= d") for fn in BOTH],
    *[(fn, dict(beta0=Q), "the rows of beta0 must be 16-byte aligned") for fn in BOTH],
    *[(fn, dict(workspace=Q), "misaligned workspace") for fn in BOTH],
    (Bk, dict(ldda=64), "ldda must be >= d"),
    (Bk, dict(dA=Q), "the rows of dA must be 16-byte aligned"),
    (Bk, dict(dZ0=None), "dZ0 and dZ1 go together"),
    (Bk, dict(dZ1=None), "dZ0 and dZ1 go together"),
    (Bk, dict(lddz1=64), "lddz0 / lddz1 must be >= d"),
    (Bk, dict(dZ0=Q), "the rows of dZ0 / dZ1 must be 16-byte aligned"),
    (Bk, dict(lddz1=258), "the rows of dZ0 / dZ1 must be 16-byte aligned"),
    (Bk, dict(dW1=None), "dW1, db1 and dW2 go together"),
    (Bk, dict(db1=None), "dW1, db1 and dW2 go together"),
    (Bk, dict(dW2=None), "dW1, db1 and dW2 go together"),
    (Bk, dict(MEAN, dW1=P, db1=P, dW2=P), "the mean of the views has no parameters"),
    (Bk, dict(dA=None, dZ0=None, dZ1=None, dW1=None, db1=None, dW2=None),
     "nothing to compute (no dA, no dZ, no parameter gradients)"),
]


def _do(lib, fn, args):
    return getattr(lib, fn)(*[args[k] for k in ORDER[fn]])


@pytest.mark.parametrize("fn,over,text", CASES,
                         ids=[f"{c[0][12:]}-{'-'.join(c[1])}-{i}" for i, c in enumerate(CASES)])
def test_rejection(fn, over, text):
    lib = _native.load()
    assert _do(lib, fn, dict(VALID[fn], **over)) == INVALID
    assert lib.hgd_get_last_error_string().decode() == f"{fn}: {text}"


def test_workspace_too_small():
    lib = _native.load()
    size = lib.hgd_cf_loss_workspace_size
    need_f, need_b = size(64, 128, 0), size(64, 128, 1)
    assert 0 < need_f < need_b and need_b - need_f >= 6 * 128 * 128 * 4
    for fn, need in ((Fw, need_f), (Bk, need_b)):
        assert _do(lib, fn, dict(VALID[fn], workspace_bytes=need - 1)) == WORKSPACE
        assert lib.hgd_get_last_error_string().decode() == \
            f"{fn}: workspace {need - 1} < required {need}"
        assert _do(lib, fn, dict(VALID[fn], workspace=None)) == WORKSPACE
        assert lib.hgd_get_last_error_string().decode() == \
            f"{fn}: workspace 0 < required {need}"


def test_empty_batch_is_accepted_without_a_launch():
    lib = _native.load()
    for fn in BOTH:
        assert _do(lib, fn, dict(VALID[fn], batch=0)) == OK
        assert _do(lib, fn, dict(VALID[fn], **MEAN, batch=0, d=200, ldu=200, ld0=200,
                                 ld1=400, ldda=200, lddz0=200, lddz1=200)) == OK
        # ... and is still validated
        assert _do(lib, fn, dict(VALID[fn], batch=0, U=None)) == INVALID


def test_workspace_size():
    size = _native.load().hgd_cf_loss_workspace_size
    assert size(0, 128, 0) == 0 and size(-5, 128, 1) == 0
    assert size(64, 20, 1) == 0 and size(64, 144, 1) == 0 and size(64, 18, 0) == 0
    assert size(64, 200, 0) > 0 and size(64, 200, 1) == 0
    for d in (16, 48, 128):
        sizes = [size(B, d, 1) for B in (1, 15, 16, 17, 2048, 100000)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (d, sizes)
        assert sizes[-1] >= 6 * 2 * 100000 * d * 4
        # the forward's share: the blocks' partial sums, O(B / 16)
        assert size(2048, d, 0) <= 4096
