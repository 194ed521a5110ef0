"""CPU: what hgd_adam_step answers to a call it rejects. Every check runs before the first HIP
call, so the device pointers are small fake integers and no device is needed; the tensor list is
a host array and is a real one. tests/test_gpu_adam_edges.py repeats the refusals with real
buffers and checks that none was written."""
import ctypes

import pytest

from hypergraph_diffusion_for_recommendation_amd import _native as nat

OK, INVALID = 0, 1  # HGD_OK, HGD_ERR_INVALID_ARG
P = 16  # a fake, 16-byte aligned, never dereferenced pointer
FIELDS = ("param", "grad", "exp_avg", "exp_avg_sq")


def _list(count, **edit):
    arr = (nat.AdamTensor * max(count, 1))()
    for t in range(count):
        for f in FIELDS:
            setattr(arr[t], f, P)
        arr[t].n = 8
    for key, value in edit.items():  # "grad_3" = None: field of tensor 3
        f, t = key.rsplit("_", 1)
        setattr(arr[int(t)], f, value)
    return arr


def _call(arr, count, scalars=P, step_row=P, variant=0):
    lib = nat.load()
    st = lib.hgd_adam_step(ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, count,
                           scalars, step_row, variant, None)
    return st, lib.hgd_get_last_error_string().decode()


CASES = [
    ("count0", dict(arr=_list(0), count=0), "1 to 16 tensors"),
    ("count-1", dict(arr=_list(1), count=-1), "1 to 16 tensors"),
    ("count17", dict(arr=_list(17), count=17), "1 to 16 tensors"),
    ("null-list", dict(arr=None, count=4), "1 to 16 tensors"),
    ("variant-1", dict(arr=_list(4), count=4, variant=-1), "variant in [0, 32)"),
    ("variant32", dict(arr=_list(4), count=4, variant=32), "variant in [0, 32)"),
    ("null-scalars", dict(arr=_list(4), count=4, scalars=None), "null scalars"),
    ("negative-n", dict(arr=_list(4, n_2=-1), count=4), "tensor 2 has a negative size"),
    ("negative-n-last", dict(arr=_list(16, n_15=-(2 ** 40)), count=16),
     "tensor 15 has a negative size"),
    *[(f"null-{f}", dict(arr=_list(4, **{f"{f}_{t}": None}), count=4),
       f"tensor {t} has a null pointer") for t, f in enumerate(FIELDS)],
]


@pytest.mark.parametrize("name,args,text", CASES, ids=[c[0] for c in CASES])
def test_rejection(name, args, text):
    status, message = _call(**args)
    assert status == INVALID
    assert message == f"hgd_adam_step: {text}"


def test_the_first_bad_tensor_is_named():
    status, message = _call(_list(16, grad_9=None, n_12=-1), 16)
    assert status == INVALID and message == "hgd_adam_step: tensor 9 has a null pointer"


def test_an_all_empty_launch_with_null_arrays_is_accepted():
    """n == 0 needs no array, and with no element and a NULL step_row nothing is launched: the
    only accepted call that a machine without a device can make."""
    arr = (nat.AdamTensor * 16)()
    for count in (1, 16):
        assert _call(arr, count, step_row=None, variant=31) == (OK, "")
