"""CPU: what the evaluation entry points (hgd_topk_rows, hgd_mask_scores, hgd_rank_metrics) answer
to a call they reject. Argument validation only: every case returns before the first HIP call, so
the device pointers are small fake integers and no device is needed (the metrics' cut-off list is
a HOST array and is a real one). Each case pins the hgd_status named in include/hgd.h and a
message prefixed with the entry's name."""
import ctypes

import pytest

from hypergraph_diffusion_for_recommendation_amd import _native

OK, INVALID, UNSUPPORTED = 0, 1, 3  # HGD_OK, HGD_ERR_INVALID_ARG, HGD_ERR_UNSUPPORTED
P = 16  # a fake, 16-byte aligned, never dereferenced pointer

T, M, R = "hgd_topk_rows", "hgd_mask_scores", "hgd_rank_metrics"
ORDER = {
    T: ["scores", "n_rows", "n_cols", "ld", "k", "out_ids", "out_scores", "stream"],
    M: ["scores", "n_rows", "ld", "rowptr", "cols", "row_map", "value", "stream"],
    R: ["ids", "n_rows", "ld", "k", "test_rowptr", "test_cols", "cutoffs", "n_cutoffs",
        "discount", "hits", "dcg", "stream"],
}
VALID = {
    T: dict(scores=P, n_rows=24, n_cols=301, ld=304, k=20, out_ids=P, out_scores=P, stream=None),
    M: dict(scores=P, n_rows=24, ld=304, rowptr=P, cols=P, row_map=P, value=-10e8, stream=None),
    R: dict(ids=P, n_rows=24, ld=24, k=20, test_rowptr=P, test_cols=P, cutoffs=[10, 20],
            n_cutoffs=None, discount=P, hits=P, dcg=P, stream=None),
}
CUT = "cut-offs must be ascending in [1, k=20]"

CASES = [
    # negative sizes
    (T, dict(n_rows=-1), INVALID, "sizes"),
    (T, dict(n_cols=-1, ld=-1), INVALID, "sizes"),
    (T, dict(n_rows=-1, scores=None), INVALID, "sizes"),
    (M, dict(n_rows=-1), INVALID, "sizes"),
    (M, dict(ld=0), INVALID, "sizes"),
    (M, dict(ld=-304), INVALID, "sizes"),
    (R, dict(n_rows=-1), INVALID, "bad n_rows / ld"),
    # a leading dimension below the row
    (T, dict(ld=300), INVALID, "sizes"),
    (T, dict(ld=0), INVALID, "sizes"),
    (R, dict(ld=19), INVALID, "bad n_rows / ld"),
    (R, dict(ld=0), INVALID, "bad n_rows / ld"),
    # k outside [1, 256]
    (T, dict(k=0), INVALID, "k must be in [1, 256]"),
    (T, dict(k=-1), INVALID, "k must be in [1, 256]"),
    (T, dict(k=257), INVALID, "k must be in [1, 256]"),
    (T, dict(k=257, n_cols=300, ld=300, n_rows=0), INVALID, "k must be in [1, 256]"),
    (R, dict(k=0), INVALID, "k must be in [1, 256] (got 0)"),
    (R, dict(k=257, ld=257), INVALID, "k must be in [1, 256] (got 257)"),
    # fewer columns than k
    (T, dict(n_cols=19, ld=19), INVALID, "fewer columns (19) than k (20)"),
    (T, dict(n_cols=0), INVALID, "fewer columns (0) than k (20)"),
    (T, dict(n_cols=255, k=256, n_rows=0), INVALID, "fewer columns (255) than k (256)"),
    # null pointers with n_rows > 0
    *[(T, {a: None}, INVALID, "null pointer") for a in ("scores", "out_ids", "out_scores")],
    *[(M, {a: None}, INVALID, "null pointer") for a in ("scores", "rowptr")],
    *[(R, {a: None}, INVALID, "null pointer")
      for a in ("ids", "test_rowptr", "discount", "hits", "dcg")],
    # n_rows = 0 launches nothing, whatever the pointers
    (T, dict(n_rows=0, scores=None, out_ids=None, out_scores=None), OK, ""),
    (T, dict(n_rows=0, n_cols=20, ld=20), OK, ""),
    (M, dict(n_rows=0, scores=None, rowptr=None, cols=None, row_map=None), OK, ""),
    (R, dict(n_rows=0, ids=None, test_rowptr=None, test_cols=None, discount=None, hits=None,
             dcg=None), OK, ""),
    # one block per row: more rows than a grid holds
    (T, dict(n_rows=2 ** 31), UNSUPPORTED, "too many rows"),
    (M, dict(n_rows=2 ** 31), UNSUPPORTED, "too many rows"),
    (R, dict(n_rows=2 ** 31), UNSUPPORTED, "too many rows"),
    (T, dict(n_rows=2 ** 40), UNSUPPORTED, "too many rows"),
    (M, dict(n_rows=2 ** 40), UNSUPPORTED, "too many rows"),
    (R, dict(n_rows=2 ** 40), UNSUPPORTED, "too many rows"),
    # the metrics' cut-off list (a host array)
    (R, dict(cutoffs=None), INVALID, "need 1..16 cut-offs (got 2)"),
    (R, dict(cutoffs=[]), INVALID, "need 1..16 cut-offs (got 0)"),
    (R, dict(cutoffs=[10], n_cutoffs=-1), INVALID, "need 1..16 cut-offs (got -1)"),
    (R, dict(cutoffs=list(range(1, 18))), INVALID, "need 1..16 cut-offs (got 17)"),
    (R, dict(cutoffs=[20, 10]), INVALID, f"{CUT} (cutoffs[1]=10)"),
    (R, dict(cutoffs=[10, 10]), INVALID, f"{CUT} (cutoffs[1]=10)"),
    (R, dict(cutoffs=[10, 21]), INVALID, f"{CUT} (cutoffs[1]=21)"),
    (R, dict(cutoffs=[0, 10]), INVALID, f"{CUT} (cutoffs[0]=0)"),
    (R, dict(cutoffs=[-5]), INVALID, f"{CUT} (cutoffs[0]=-5)"),
    (R, dict(cutoffs=[1, 2, 3, 20, 4]), INVALID, f"{CUT} (cutoffs[4]=4)"),
    # a bad cut-off list is refused even for an empty batch; 16 cut-offs up to k are accepted
    (R, dict(cutoffs=[20, 10], n_rows=0), INVALID, f"{CUT} (cutoffs[1]=10)"),
    (R, dict(cutoffs=list(range(5, 21)), n_rows=0), OK, ""),
    (R, dict(cutoffs=[20], n_rows=0, ids=None), OK, ""),
]


def _call(lib, fn, over):
    args = dict(VALID[fn], **over)
    if fn == R:
        cut = args["cutoffs"]
        if args["n_cutoffs"] is None:
            args["n_cutoffs"] = 2 if cut is None else len(cut)
        # one spare element: an empty list still hands the entry a real host pointer
        args["cutoffs"] = None if cut is None else (ctypes.c_int32 * (len(cut) + 1))(*cut)
    return getattr(lib, fn)(*[args[a] for a in ORDER[fn]])


@pytest.mark.parametrize("fn,over,status,text", CASES,
                         ids=[f"{c[0][4:]}-{'-'.join(c[1])}-{i}" for i, c in enumerate(CASES)])
def test_rejection(fn, over, status, text):
    lib = _native.load()
    assert _call(lib, fn, over) == status
    assert lib.hgd_get_last_error_string().decode() == (f"{fn}: {text}" if text else "")


def test_valid_tables_are_what_the_cases_vary():
    """The unvaried arguments pass every check: with n_rows = 0 (nothing launched) each VALID
    table answers HGD_OK, so a case's status comes from the argument it overrides."""
    lib = _native.load()
    for fn in (T, M, R):
        assert _call(lib, fn, dict(n_rows=0)) == OK
        assert lib.hgd_get_last_error_string().decode() == ""


def test_python_surface_refuses_before_launch():
    import torch
    from hypergraph_diffusion_for_recommendation_amd.evaluation import rank_metrics, topk_rows
    for bad in (torch.zeros(4, 30), torch.zeros(30), torch.zeros(4, 30, dtype=torch.float64)):
        with pytest.raises(TypeError, match="2-D float32 device tensor"):
            topk_rows(bad, 5)
    with pytest.raises(TypeError, match="2-D int32 device tensor"):
        rank_metrics(torch.zeros(4, 10, dtype=torch.int32), None, [5])
