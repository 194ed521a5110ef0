"""CPU: the numpy model and the input builders of tests/_rank_ref.py (the streaming rule of
csrc/rank.hip). The model's merged lists must be the closed form of find_k_largest for every
content family, k and segment count; the builders must reach the branches they name."""
import numpy as np
import pytest

from tests import _rank_ref as R
from tests import _topk_ref as T


def _finite_mixed(n_cols, k):
    S = T.mixed_rows(n_cols, k)
    return S + np.float32(0.0)  # -0.0 → +0.0, as the embeddings of from_rows give them


@pytest.mark.parametrize("n_segments", [1, 2, 3, 7, 1000])
@pytest.mark.parametrize("n_cols,k", [(64, 64), (65, 64), (63, 20), (129, 1), (579, 40),
                                      (579, 63), (200, 2)])
def test_model_equals_closed_form(n_cols, k, n_segments):
    nseg = R.segments_for(12, n_cols, n_segments)
    assert nseg == min(n_segments, R.n_tiles(n_cols))
    for row in _finite_mixed(n_cols, k):
        segs = R.plan(row, k, nseg)
        assert len(segs) == nseg
        ids, sc = R.merged(row, k, segs)
        ref_ids, ref_bits = T.expected(row, k)
        assert ids == ref_ids
        assert T.bits(np.asarray(sc, np.float32)).tolist() == ref_bits.tolist()


@pytest.mark.parametrize("kind", ["inf", "zero", "masked"])
def test_model_on_special_rows(kind):
    for k in (1, 20, 64):
        for row in T.special_rows(kind, 300, k):
            for nseg in (1, 3):
                ids, sc = R.merged(row, k, R.plan(row, k, nseg))
                ref_ids, _ = T.expected(row, k)
                assert ids == ref_ids


def test_model_with_masked_rows():
    """Filtering on the raw score and masking at the compaction gives the closed form of the
    effective row, also when every raw score is below the mask value."""
    for ue, ie, rated in (
            (*R.integer_case(6, 5 * R.TI + 7, 8), R.random_rated(6, 5 * R.TI + 7, 0.3,
                                                                 everything=(1,), nothing=(0,))),
            (*R.below_mask_case(6, 5 * R.TI + 7), R.random_rated(6, 5 * R.TI + 7, 0.02,
                                                                 everything=(1,), nothing=(0,)))):
        users = np.arange(6)
        E = R.effective(ue, ie, users, rated)
        raw = R.effective(ue, ie, users, [np.zeros(0, np.int32)] * 6)
        for k in (1, 20, 64):
            for nseg in (1, 2, 6):
                for r in range(6):
                    segs = R.plan(E[r], k, nseg, row_raw=raw[r])
                    ids, _ = R.merged(E[r], k, segs)
                    assert ids == T.expected(E[r], k)[0]


def test_segments():
    assert R.segment_tiles(9 * R.TI + 3, 3) == [(0, 4), (4, 8), (8, 10)]
    assert R.segment_tiles(10 * R.TI, 7) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 10),
                                             (10, 10)]  # late segments may be empty
    # by shape: two workgroups per CU of 256, at least 8 tiles each, at most 256
    assert R.segments_for(64, 1_000_000, 0) == 256
    assert R.segments_for(65_536, 1_000_000, 0) == 1
    assert R.segments_for(31_668, 38_048, 0) == 2
    assert R.segments_for(64, 10 * R.TI, 0) == 1
    assert R.segments_for(1, 64 * R.TI, 0) == 8
    assert R.segments_for(1, 100, 5) == 2 and R.segments_for(1, 64, 0) == 1


@pytest.mark.parametrize("k", [1, 20, R.MAX_K])
def test_compaction_builders(k):
    TI = R.TI
    assert R.branch(R.plan(R.compaction_row(TI, k, "none"), k, 1)) == {"none"}
    assert "one" in R.branch(R.plan(R.compaction_row(TI + 1, k, "one"), k, 1))
    assert "one" in R.branch(R.plan(R.compaction_row(9 * TI + 3, k, "one"), k, 1))
    segs = R.plan(R.compaction_row(9 * TI + 3, k, "several"), k, 1)
    # (the 3 items of the partial tile overflow SLOTS - TI only on top of more than 61 held)
    assert segs[0]["compactions"] == list(range(1, 9)) + ([9] if k + 3 > R.SLOTS - TI else [])
    assert segs[0]["appends"] == 9 * TI + 3
    segs = R.plan(R.compaction_row(4 * TI, k, "last_tile"), k, 1)
    assert segs[0]["compactions"] == [1, 3]
    if k > 1:  # k = 1: a partial tile's 63 items on top of 1 held never exceed SLOTS - TI
        n = 3 * TI + (TI - k + 1)
        segs = R.plan(R.compaction_row(n, k, "partial_tile"), k, 1)
        assert segs[0]["compactions"] == [1, 3] and n % TI
    # the same ascending row over 3 segments: a compaction in each segment's last tile
    segs = R.plan(R.compaction_row(9 * TI + 3, k, "several"), k, 3)
    assert "last_tile" in R.branch(segs) and [s["tiles"] for s in segs] == [(0, 4), (4, 8), (8, 10)]


def test_exact_embeddings():
    S = _finite_mixed(200, 20)
    ue, ie = R.from_rows(S, 16)
    users = np.arange(len(S))
    none = [np.zeros(0, np.int32)] * len(S)
    assert np.array_equal(T.bits(R.effective(ue, ie, users, none)), T.bits(S))
    ue, ie = R.integer_case(7, 130, 33)
    rated = R.random_rated(7, 130, 0.2, everything=(2,), nothing=(3,), duplicate=(4,))
    E = R.effective(ue, ie, np.arange(7), rated)
    assert (E[2] == R.MASK_VALUE).all() and not (E[3] == R.MASK_VALUE).any()
    rowptr, cols = R.csr_of(rated)
    assert rowptr[-1] == len(cols) and rowptr[3] == rowptr[4]
    ue, ie = R.below_mask_case(3, 100)
    raw = R.effective(ue, ie, np.arange(3), [np.zeros(0, np.int32)] * 3)
    assert (raw < R.MASK_VALUE).all()
    E = R.effective(ue, ie, np.arange(3), R.random_rated(3, 100, 0.3))
    assert ((E == R.MASK_VALUE) | (E == raw)).all() and (E == R.MASK_VALUE).any()
    ue, ie = R.ramp_case(100)
    assert R.effective(ue, ie, [0], [[]])[0].tolist() == list(range(100))


def test_real_case_keeps_seeds_out():
    rated = R.random_rated(5, 1000, 0.05)
    ue, ie, S, bound = R.real_case(5, 1000, 64, 20, rated)
    assert (ie[:20] == 0).all() and S.shape == bound.shape == (5, 1000)
    assert (S[0, rated[0]] == float(R.MASK_VALUE)).all()
