"""Inputs and a numpy model of the streaming rule of csrc/rank.hip (hgd_rank_topk), for
tests/test_gpu_rank_fused.py. No GPU code here.

The kernel's rule, restated (``plan``): the catalogue is cut into tiles of TI items and the tiles
into ``n_segments`` contiguous runs. Inside a segment a user starts with no threshold and takes
every score; a score is appended to the user's SLOTS candidate slots when there is no threshold
yet, or the threshold is below the mask value (a rated item is raised to it), or its *raw* value
is strictly larger than the threshold *as it stood when its tile began*; after a tile, a user
holding more than SLOTS - TI candidates is compacted: the new candidates take their effective
score (the mask value if rated), all are sorted by (score desc, id asc), the first k kept, and —
once k are held — the k-th becomes the threshold. At the end each segment hands over its k best;
the merge orders them with the k seed copies (the effective scores of items 0..k-1) by (score
desc, seed first, id asc).

Builders make embeddings whose fp32 scores are exact (small integers, or one nonzero term per
score), and assert the branch they were meant to reach through ``plan``. The expected lists are
``oracle.hgd_oracle.masked_scores`` → ``topk_closed_form``, cross-checked with the literal
``find_k_largest`` on short rows (``_topk_ref.expected``). tests/test_rank_ref.py checks this
module on the CPU.
"""
import numpy as np

from oracle import hgd_oracle as O
from tests import _topk_ref as T

TU = 64        # users per workgroup
TI = 64        # items per tile
SLOTS = 128    # candidate slots per user
MAX_K = 64     # HGD_RANK_MAX_K
MAX_D = 256    # HGD_RANK_MAX_D
MAX_SEGMENTS = 256
CUS = 256      # the constant CU count of the automatic segment choice
MASK_VALUE = np.float32(-10e8)


def n_tiles(n_items):
    return -(-n_items // TI)


def segments_for(n_rows, n_items, n_segments):
    """The segment count the kernel launches: the caller's, or for 0 enough workgroups for two
    per CU with at least 8 tiles each; never more than the tiles or MAX_SEGMENTS."""
    tiles, blocks = n_tiles(n_items), -(-n_rows // TU)
    n = n_segments
    if n == 0:
        n = min(-(-2 * CUS // max(1, blocks)), tiles // 8)
    return max(1, min(n, tiles, MAX_SEGMENTS))


def segment_tiles(n_items, n_segments):
    """[(first tile, end tile)] of each of the ``n_segments`` launched segments (a late segment
    may be empty: the tiles are dealt in runs of ceil(tiles / n_segments))."""
    tiles = n_tiles(n_items)
    per = -(-tiles // n_segments)
    return [(min(tiles, s * per), min(tiles, (s + 1) * per)) for s in range(n_segments)]


def _order(cands):
    return sorted(cands, key=lambda c: (-c[0], c[1]))


def plan(row_effective, k, n_segments, row_raw=None, mask_value=MASK_VALUE):
    """The stream of one user's row of effective scores over ``n_segments`` launched segments
    (already resolved: see ``segments_for``); ``row_raw`` are the scores before masking (default:
    nothing is masked). Per segment a dict: ``tiles`` (first, end), ``appends`` (candidates that
    passed the filter), ``compactions`` (the tiles after which the user was compacted) and
    ``best`` (its k best as (score, id), fewer if it saw fewer)."""
    row = np.asarray(row_effective, dtype=np.float32)
    raw = row if row_raw is None else np.asarray(row_raw, dtype=np.float32)
    masks = row_raw is not None
    n = len(row)
    assert 1 <= k <= min(n, MAX_K) and len(raw) == n
    out = []
    for t0, t1 in segment_tiles(n, n_segments):
        tau, held, appends, compactions = None, [], 0, []
        for t in range(t0, t1):
            everything = tau is None or t == 0 or (masks and not mask_value <= tau)
            for i in range(t * TI, min(n, (t + 1) * TI)):
                if everything or raw[i] > tau:
                    held.append((float(row[i]), i))
                    appends += 1
            assert len(held) <= SLOTS
            if len(held) > SLOTS - TI:
                n_before = len(held)
                held = _order(held)[:k]
                if n_before >= k:
                    tau = np.float32(held[k - 1][0])
                compactions.append(t)
        out.append(dict(tiles=(t0, t1), appends=appends, compactions=compactions,
                        best=_order(held)[:k]))
    return out


def merged(row_effective, k, segs):
    """(ids, scores) of the merge of a ``plan``: seeds and the segments' best, by (score desc,
    seed first, id asc)."""
    row = np.asarray(row_effective, dtype=np.float32)
    cands = [(float(row[j]), 1, j) for j in range(k)]
    for s in segs:
        cands += [(sc, 0, i) for sc, i in s["best"]]
    cands.sort(key=lambda c: (-c[0], -c[1], c[2]))
    return [c[2] for c in cands[:k]], [c[0] for c in cands[:k]]


def branch(segs):
    """Which compaction branches a plan reaches: 'none', 'one', 'several' (by the largest count
    in any segment), plus 'last_tile' (a compaction after a segment's last tile) and
    'partial_tile' (after the catalogue's last, partial tile) where they occur."""
    most = max(len(s["compactions"]) for s in segs)
    got = {"none" if most == 0 else "one" if most == 1 else "several"}
    for s in segs:
        if s["compactions"] and s["compactions"][-1] == s["tiles"][1] - 1:
            got.add("last_tile")
    return got


# ---- embeddings with exact scores ------------------------------------------------------------
def effective(ue, ie, users, rated_rows, mask_value=MASK_VALUE):
    """The fp32 rows of effective scores of exact-score embeddings: the float64 oracle's masked
    scores, asserted representable in fp32 (so any summation order gives these bits); a zero is
    +0.0, as a sum from a +0.0 accumulator is."""
    S = O.masked_scores(ue, ie, users, rated_rows, float(mask_value)) + 0.0
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S), "scores are not exact in fp32"
    return S32


def expected(S32, k):
    """[(ids, score bits)] per row of effective scores (closed form; literal on short rows)."""
    return [T.expected(row, k) for row in S32]


def from_rows(S, d):
    """(ue, ie) with ue[r]·ie[i] == S[r, i] exactly: user r is the unit vector e_r (so at most d
    rows), item i holds column i of S in its first len(S) features — one nonzero term per score.
    -0.0 entries come out as +0.0 (the product is added to a +0.0 accumulator)."""
    S = np.asarray(S, dtype=np.float32)
    rows, n = S.shape
    assert rows <= d and np.isfinite(S).all()
    ue = np.zeros((rows, d), dtype=np.float32)
    ue[np.arange(rows), np.arange(rows)] = 1.0
    ie = np.zeros((n, d), dtype=np.float32)
    ie[:, :rows] = S.T
    return ue, ie


def integer_case(n_users, n_items, d, seed=0, lo=-2, hi=3):
    """Small-integer embeddings: every partial sum is an integer far below 2^24."""
    rng = np.random.default_rng([n_users, n_items, d, seed])
    return (rng.integers(lo, hi, size=(n_users, d)).astype(np.float32),
            rng.integers(lo, hi, size=(n_items, d)).astype(np.float32))


def ramp_case(n_items, descending=False):
    """d = 1, u = [1], v_i = i (or -i): ascending scores make every tile append for the user and
    compact after every tile from the second on; descending ones stop after the first k."""
    ue = np.ones((1, 1), dtype=np.float32)
    ie = np.arange(n_items, dtype=np.float32).reshape(-1, 1)
    return ue, (-ie if descending else ie)


def below_mask_case(n_users, n_items, d=4, seed=0):
    """Raw scores all far below -10e8: u_j = -2^16, v_j in {2^15, 2^15 + 2^10, ...} — products of
    powers of two and small integers, exact in fp32. A rated item is *raised* to -10e8."""
    rng = np.random.default_rng([n_users, n_items, d, seed, 7])
    ue = np.full((n_users, d), -2.0 ** 16, dtype=np.float32)
    ie = (2.0 ** 15 + 2.0 ** 10 * rng.integers(0, 8, size=(n_items, d))).astype(np.float32)
    assert (ue[:1].astype(np.float64) @ ie.T.astype(np.float64)).max() < float(MASK_VALUE)
    return ue, ie


def random_rated(n_users, n_items, density, seed=0, everything=(), nothing=(), duplicate=()):
    """Rated rows (ascending int32 arrays) per user: random at ``density``; users in
    ``everything`` rated every item, in ``nothing`` none, in ``duplicate`` have every column
    listed twice."""
    rng = np.random.default_rng([n_users, n_items, seed, 11])
    rows = []
    for u in range(n_users):
        c = np.flatnonzero(rng.random(n_items) < density)
        if u in everything:
            c = np.arange(n_items)
        if u in nothing:
            c = c[:0]
        if u in duplicate:
            c = c if len(c) else np.array([n_items // 2])
            c = np.sort(np.concatenate([c, c]))
        rows.append(c.astype(np.int32))
    for u in everything:
        assert len(rows[u]) == n_items
    for u in nothing:
        assert len(rows[u]) == 0
    for u in duplicate:
        assert len(rows[u]) and len(rows[u]) == 2 * len(np.unique(rows[u]))
    return rows


def csr_of(rated_rows):
    """(rowptr int64, cols int32) of rated rows."""
    rowptr = np.zeros(len(rated_rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rated_rows])
    cols = np.concatenate(rated_rows).astype(np.int32) if len(rated_rows) else \
        np.zeros(0, np.int32)
    return rowptr, cols


# ---- builders that sit on the compaction branches --------------------------------------------
def compaction_row(n_items, k, kind):
    """One row of integer scores (ids >= k only ever rise where said, the seed window stays low)
    whose single-segment plan takes exactly the named branch:
      "none"          a catalogue of one tile (n_items <= TI): never more than SLOTS - TI held;
      "one"           the second tile fills the slots (everything passes while no threshold is
                      set), then nothing passes again: descending scores;
      "several"       ascending scores: every tile appends TI and compacts;
      "last_tile"     descending scores except that the segment's last full tile ascends above
                      everything, filling the slots again there;
      "partial_tile"  as "last_tile" with the rise in the catalogue's last, partial tile (needs
                      n_items % TI > SLOTS - TI - k)."""
    idx = np.arange(n_items, dtype=np.float32)
    if kind == "none":
        assert n_items <= TI
        row = idx.copy()
    elif kind == "one":
        assert n_items > TI
        row = -idx
    elif kind == "several":
        assert n_items > 2 * TI
        row = idx.copy()
    elif kind in ("last_tile", "partial_tile"):
        row = -idx
        t_last = n_tiles(n_items) - 1
        lo = t_last * TI
        if kind == "partial_tile":
            assert n_items % TI and n_items - lo > SLOTS - TI - k and t_last >= 2
        else:
            assert n_items % TI == 0 and t_last >= 2
        row[lo:] = 10.0 + np.arange(n_items - lo)
    else:
        raise ValueError(kind)
    segs = plan(row, k, 1)
    got = branch(segs)
    if kind in ("none", "one", "several"):
        assert kind in got, (kind, got, segs[0]["compactions"])
    else:
        assert segs[0]["compactions"][-1] == n_tiles(n_items) - 1, segs[0]["compactions"]
        assert len(segs[0]["compactions"]) == 2
    return row


# ---- real-valued parity ----------------------------------------------------------------------
def real_case(n_users, n_items, d, k, rated_rows=None, seed=0):
    """Normal embeddings with the first k items zero, so that no seed copy reaches a list: the
    builder asserts that every user's k-th largest float64 effective score exceeds 0 by more
    than the bound. Returns (ue, ie, S64 effective scores, bound = RTOL·Σ|terms|)."""
    from tests._util import RTOL
    rng = np.random.default_rng([n_users, n_items, d, k, seed])
    ue = rng.standard_normal((n_users, d)).astype(np.float32)
    ie = rng.standard_normal((n_items, d)).astype(np.float32)
    ie[:k] = 0.0
    S = ue.astype(np.float64) @ ie.astype(np.float64).T
    bound = RTOL * (np.abs(ue).astype(np.float64) @ np.abs(ie).astype(np.float64).T)
    if rated_rows is not None:
        for u, cols in enumerate(rated_rows):
            S[u, cols] = float(MASK_VALUE)
    kth = -np.sort(-S, axis=1)[:, k - 1]
    assert (kth > bound.max()).all(), "a seed copy (score 0) could reach a list"
    return ue, ie, S, bound
