"""Inputs and numpy restatements for the unique and device graph-build edge tests
(tests/test_gpu_unique_edges.py, tests/test_gpu_ingest_edges.py). No GPU code here.

Unique (csrc/unique.hip): key lists whose sorted distinct values are known by construction, so
that a 2^24-key case needs no host sort, placed on the guards of the range bitmap (32-bit words,
8 words per thread, 2,048-word tiles, the 1,024-word LDS bitmap, the 2^24-bit window) and of the
far-key sort (4,096 keys in LDS, 1,024-wide chunks of the distinct pass). tests/test_unique_ref.py
checks every construction against ``np.unique`` at the sizes a host sort handles.

Graph build (csrc/ingest.hip): the dict loop of ``Interaction.__generate_set``
(data/ui_graph.py:43-56), scipy's canonical ``csr_matrix((ones, (row, col)))`` restated through
``np.unique`` on the int64 key, and the float32 products of ``Graph.normalize_graph_mat``
(data/graph.py:11-25).
"""
import numpy as np

INT64_MIN = -2 ** 63
INT64_MAX = 2 ** 63 - 1

WORD = 32                      # bits per bitmap word
WORDS_PER_THREAD = 8           # kWordsPerThread
TILE_WORDS = 2048              # kTileWords
TILE_BITS = TILE_WORDS * WORD  # 65,536 keys per tile
LDS_WORDS = 1024               # kLdsWords: block-private bitmap up to this many words
CAP_BITS = 1 << 24             # kCapBits: the bitmap window
MAX_TILES = 256                # kMaxTiles
FAR_LDS = 4096                 # kFarLds: far keys sorted in LDS up to this many
FAR_THREADS = 1024             # kFarThreads: chunk of the distinct pass
LOS = (-3, 2 ** 40 + 5)        # window starts: next to 0 and far from it


# ---------------------------------------------------------------- restatements
def trunc_long(x_f32):
    """``Tensor.long()`` of float32 values as TruncSrc (csrc/unique.hip) documents it: truncation
    toward zero; NaN, ±inf and |x| >= 2^63 map to INT64_MIN. The integer conversion is only
    applied to values already truncated and inside the int64 range, where it is exact."""
    x = np.asarray(x_f32, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x) < np.float32(2.0 ** 63)  # False for NaN and ±inf
    t = np.trunc(np.where(ok, x, np.float32(0))).astype(np.int64)
    return np.where(ok, t, np.int64(INT64_MIN))


def unique_ref(keys_i64):
    keys = np.asarray(keys_i64)
    assert keys.dtype == np.int64
    return np.unique(keys)


def same_list(got, want):
    """The comparison every unique test uses: ``got`` (a tensor) is int64 and holds exactly the
    values of ``want`` (numpy or tensor) in the same order — bit-exact, no tolerance."""
    import torch
    want = torch.as_tensor(want)
    return (got.dtype == torch.int64 and want.dtype == torch.int64 and got.dim() == 1
            and got.shape == want.shape and torch.equal(got, want.to(got.device)))


def perturbed(expected):
    """Three wrong answers a slipped guard would give: one element dropped, one duplicated, one
    adjacent pair swapped (``expected`` needs two elements or more)."""
    e = np.asarray(expected)
    assert e.size >= 2
    m = e.size // 2
    swap = e.copy()
    swap[[m - 1, m]] = swap[[m, m - 1]]
    return {"dropped": np.delete(e, m), "duplicated": np.insert(e, m, e[m]), "swapped": swap}


# ---------------------------------------------------------------- unique input builders
def _offset(lo, pos):
    pos = np.asarray(pos, dtype=np.int64)
    assert pos.min(initial=0) >= 0 and lo + int(pos.max(initial=0)) <= INT64_MAX
    return np.int64(lo) + pos


def bits_at(lo, bit_positions, repeats=1, seed=0):
    """``(keys, expected)``: the keys ``lo + position``, each ``repeats`` times (an int, or one
    count per position), shuffled; expected is ``lo + sorted distinct positions``."""
    pos = np.unique(np.asarray(bit_positions, dtype=np.int64))
    rep = np.broadcast_to(np.asarray(repeats, dtype=np.int64), pos.shape)
    assert pos.size and (rep >= 1).all()
    keys = _offset(lo, np.repeat(pos, rep))
    np.random.default_rng(seed).shuffle(keys)
    return keys, _offset(lo, pos)


def dense(lo, n_bits, stride=1):
    """``(keys, expected)``: ``lo + i·stride`` for i < n_bits, the keys in descending order (no
    shuffle: the full window is 2^24 keys); expected ascending."""
    exp = _offset(lo, np.arange(n_bits, dtype=np.int64) * stride)
    return exp[::-1].copy(), exp


def with_far(near, far, seed=0):
    """``(keys, expected)`` of a near part (a builder's pair) and far keys, every far key above
    every near key (copies allowed): shuffled together; expected = near's, then the distinct far
    keys ascending."""
    nk, ne = near
    far = np.asarray(far, dtype=np.int64)
    assert far.size and far.min() > ne[-1]
    keys = np.concatenate([nk, far])
    np.random.default_rng(seed).shuffle(keys)
    fs = np.sort(far)
    return keys, np.concatenate([ne, fs[np.concatenate([[True], fs[1:] != fs[:-1]])]])


def sized_input(n, lo):
    """``(keys, expected)`` of exactly n keys for the grid-size cases: the minimum ``lo`` is the
    LAST element and the maximum the one before it, so a grid that stops short of the input's end
    loses a window edge. The interior is the set lo+1 .. lo+m visited in a stride-7919 order."""
    if n == 1:
        return _offset(lo, [0]), _offset(lo, [0])
    m = min(n - 2, 5000)
    inner = 1 + (np.arange(n - 2, dtype=np.int64) * 7919) % max(m, 1)  # 7919 prime, m < 7919
    hi = m + 50
    keys = _offset(lo, np.concatenate([inner, [hi, 0]]).astype(np.int64))
    exp = _offset(lo, np.concatenate([np.arange(0, m + 1), [hi]]).astype(np.int64))
    return keys, exp


def far_keys(lo, k, copies=(1,), gap=(1 << 33) + 1):
    """k distinct far keys lo + 2^24 + j·gap (the first is the first key past the window), key j
    repeated ``copies[j % len(copies)]`` times."""
    vals = _offset(lo, CAP_BITS + np.arange(k, dtype=np.int64) * gap)
    rep = np.resize(np.asarray(copies, dtype=np.int64), k)
    return np.repeat(vals, rep)


# ---- the named cases of tests/test_gpu_unique_edges.py (thunks: built when a test asks)
def _spread(rng, last, count):
    return rng.integers(0, last + 1, size=count)


def geometry_cases():
    """{name: thunk -> (keys, expected, guard)} on the bitmap's word, thread, tile and LDS
    boundaries, for both window starts. ``guard`` names the constant in csrc/unique.hip."""
    cases = {}
    for lo in LOS:
        tag = "lo%d" % (0 if lo < 0 else 40)
        for last in (0, 30, 31, 32, 63, 255, 256, 257):
            pos = sorted({0, last // 2, max(last - 1, 0), last})
            cases[f"lastbit{last}-{tag}"] = (
                lambda lo=lo, pos=pos, last=last: bits_at(lo, pos, 3, seed=last)
                + ("range_words (span + 1 + 31) / 32; w0 + j < words at kWordsPerThread",))
        for words in (1023, 1024, 1025):
            def lds(lo=lo, words=words):
                last = words * WORD - 1
                rng = np.random.default_rng(words)
                pos = [0, 31, (LDS_WORDS - 1) * WORD - 1, (LDS_WORDS - 1) * WORD,
                       LDS_WORDS * WORD - 1, LDS_WORDS * WORD, (words - 1) * WORD, last]
                pos = [p for p in pos if p <= last] + list(_spread(rng, last, 300))
                return bits_at(lo, pos, 2, seed=words) + ("words <= kLdsWords in uq_mark",)
            cases[f"words{words}-{tag}"] = lds
        for words in (2047, 2048, 2049, 4096, 4097):
            def tiles(lo=lo, words=words, mid_empty=False):
                last = words * WORD - 1
                rng = np.random.default_rng(words)
                pos = [0, TILE_BITS - 1, last] + list(_spread(rng, min(last, TILE_BITS - 1), 100))
                if not mid_empty:
                    pos.append(TILE_BITS)
                else:
                    pos.append(2 * TILE_BITS)
                pos = [p for p in pos if p <= last]
                return bits_at(lo, pos, 2, seed=words) + (
                    "tiles = ceil(words / kTileWords); tile_off of uq_scan",)
            cases[f"words{words}-{tag}"] = tiles
            if words == 4097:  # three tiles, the middle one empty: its offset stands still
                cases[f"words{words}-mid-empty-{tag}"] = (
                    lambda lo=lo, words=words, f=tiles: f(lo, words, True))

        def sparse_window(lo=lo):
            pos = [0, TILE_BITS - 1, CAP_BITS - 1] + [t * TILE_BITS for t in range(MAX_TILES)]
            return bits_at(lo, pos, 2, seed=5) + ("kCapBits - 1 span, kMaxTiles tiles",)
        cases[f"window-sparse-{tag}"] = sparse_window

        def dense_tile(lo=lo):
            pos = np.concatenate([[5], np.arange(TILE_BITS, 2 * TILE_BITS), [2 * TILE_BITS + 7]])
            return bits_at(lo, pos, 1, seed=6) + (
                "a 65,536-key tile between one-key tiles: block_exclusive_scan, tile_off",)
        cases[f"dense-tile-{tag}"] = dense_tile
    return cases


SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 131072, 131073, 2097152 + 257)
FAR_COUNTS = (1, 2, 3, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8193)


def _near(lo, seed=0):
    return bits_at(lo, [0, 1, 5, CAP_BITS - 1], 2, seed=seed)


def far_cases():
    """{name: thunk -> (keys, expected, guard)} on the window edge and the far-key sort."""
    cases = {}
    for lo in LOS:
        tag = "lo%d" % (0 if lo < 0 else 40)
        cases[f"edge-inside-{tag}"] = lambda lo=lo: bits_at(lo, [0, 7, CAP_BITS - 1], 2) + (
            "span >= kCapBits in range_words",)
        cases[f"edge-first-far-{tag}"] = lambda lo=lo: with_far(
            bits_at(lo, [0, 7], 2), far_keys(lo, 1, (2,))) + ("b >= kCapBits in uq_mark",)
        cases[f"edge-both-{tag}"] = lambda lo=lo: with_far(
            _near(lo), far_keys(lo, 1, (2,))) + ("b >= kCapBits in uq_mark",)
    for k in FAR_COUNTS:
        # one copy each: the far list is exactly k entries (LDS sort up to kFarLds, P = k at the
        # powers of two); 1 to 3 copies: runs of equal keys lie over sorted positions 1,023/1,024
        # and 4,095/4,096 (cycle of 6 entries per 3 keys: 1,020 and 4,092 start a cycle, the
        # cycle's third key covers +3 .. +5)
        cases[f"far{k}-single"] = lambda k=k: with_far(
            _near(LOS[0], k), far_keys(LOS[0], k), seed=k) + (
            "P <= kFarLds; while (P < k); c0 += kFarThreads",)
        cases[f"far{k}-copies"] = lambda k=k: with_far(
            _near(LOS[1], k), far_keys(LOS[1], k, (1, 2, 3)), seed=k) + (
            "prev = keys[i - 1] at a chunk start of the distinct pass",)
    for total in (1500, 5000):
        cases[f"far-all-equal-{total}"] = lambda total=total: with_far(
            _near(LOS[0]), far_keys(LOS[0], 1, (total,))) + ("f = v != prev over one run",)

    def max_lds():
        far = np.concatenate([far_keys(0, 3, (1, 2, 1)), [INT64_MAX, INT64_MAX]])
        return with_far(_near(0), far) + ("LLONG_MAX pad of the LDS sort, k = 6 < P = 8",)

    def max_ws():
        far = np.concatenate([far_keys(0, FAR_LDS), [INT64_MAX]])
        return with_far(_near(0), far) + ("LLONG_MAX pad of far[k, P), k = 4,097 < P = 8,192",)
    cases["far-int64-max-lds"] = max_lds
    cases["far-int64-max-workspace"] = max_ws
    cases["lo-int64-min"] = lambda: with_far(
        bits_at(INT64_MIN, [0, 3, CAP_BITS - 1], 2), far_keys(INT64_MIN, 2, (1, 2))) + (
        "unsigned key - lo with lo = INT64_MIN",)
    cases["lo-int64-min-hi-int64-max"] = lambda: with_far(
        bits_at(INT64_MIN, [0, CAP_BITS - 1], 2),
        np.concatenate([far_keys(INT64_MIN, 1), [-1, 0, INT64_MAX]])) + (
        "span = 2^64 - 1 in unsigned arithmetic",)
    return cases


F63 = 2.0 ** 63 - 2.0 ** 39  # the largest float32 below 2^63


def float_cases():
    """{name: (float32 values, guard)}: floats whose truncation lands on the same edges; the
    expected list is ``unique_ref(trunc_long(values))``."""
    nan, inf = float("nan"), float("inf")
    below1 = float(np.nextafter(np.float32(1), np.float32(0)))
    ints = bits_at(-3, [0, 2, 3, 4, (LDS_WORDS - 1) * WORD + 2, LDS_WORDS * WORD + 2,
                        LDS_WORDS * WORD + 40], 50, seed=9)[0].astype(np.float32)
    frac = np.where(ints < 0, ints - 0.5, ints + 0.5)  # |k| + 0.5 is exact in float32 here
    cases = {
        "zeros": ([0.999, -0.999, below1, -below1, -0.0, 0.0, 0.5, -0.5, 1e-42, -1e-42],
                  "static_cast<int64_t>(x) truncates toward zero"),
        "window-edge": ([0.999, -0.0, 16777215.0, 16777216.0, 16777215.0, 3.7],
                        "2^24 - 1 inside the window, 2^24 the first far key"),
        "window-inside": ([-0.999, 16777215.0, 1.5, 16777214.0], "span = kCapBits - 1"),
        "near-2^63": ([F63, -F63, 0.0, F63, -1.5, 1.5], "|x| < 2^63 in TruncSrc"),
        "all-indefinite": ([2.0 ** 63, -2.0 ** 63 - 2.0 ** 40, nan, inf, -inf, -2.0 ** 63],
                           "!(fabsf(x) < 2^63) -> INT64_MIN"),
        "indefinite-and-others": ([nan, 4.5, inf, -F63, F63, -inf, 2.0 ** 63, -7.9, 4.2],
                                  "INT64_MIN drags the window: every other key is far"),
        "lds-switch": (frac, "words <= kLdsWords with a float source"),
    }
    return {k: (np.asarray(v, dtype=np.float32), g) for k, (v, g) in cases.items()}


# ---------------------------------------------------------------- graph build restatements
def remap_ref(keys):
    """(ids int32 [n], uniq int64): the dict loop of Interaction.__generate_set."""
    seen = {}
    ids = np.empty(len(keys), dtype=np.int32)
    for i, k in enumerate(np.asarray(keys, dtype=np.int64).tolist()):
        if k not in seen:
            seen[k] = len(seen)
        ids[i] = seen[k]
    return ids, np.fromiter(seen.keys(), dtype=np.int64, count=len(seen))


def coalesce_runs_ref(rows, cols, n_cols):
    """(run rows int64, col int32, val float32) of the distinct (row, col) cells ascending by
    row·n_cols + col, the counts as float32 (the float32 sum of that many ones)."""
    key = np.asarray(rows, dtype=np.int64) * np.int64(n_cols) + np.asarray(cols, dtype=np.int64)
    uniq, counts = np.unique(key, return_counts=True)
    return uniq // n_cols, (uniq % n_cols).astype(np.int32), counts.astype(np.float32)


def coalesce_ref(rows, cols, n_rows, n_cols):
    """Canonical CSR (rowptr int64 [n_rows + 1], col int32, val float32) with summed counts."""
    rr, col, val = coalesce_runs_ref(rows, cols, n_cols)
    rowptr = np.searchsorted(rr, np.arange(n_rows + 1, dtype=np.int64), side="left")
    return rowptr.astype(np.int64), col, val


def normalize_ref(rowptr, col, val, dr, dc):
    """float32 ``(dr[r]·val[e])·dc[col[e]]`` in that order, element by element (``dc`` None: the
    rectangular case, no second factor)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    out = np.asarray(dr, dtype=np.float32)[rows] * np.asarray(val, dtype=np.float32)
    if dc is not None:
        out = out * np.asarray(dc, dtype=np.float32)[np.asarray(col)]
    assert out.dtype == np.float32
    return out


def keys_with_distinct(n, d, seed):
    """n int64 keys with exactly d distinct values drawn over the whole signed range."""
    assert 1 <= d <= n
    rng = np.random.default_rng(seed)
    vals = np.unique(rng.integers(INT64_MIN, INT64_MAX, size=2 * d + 8, dtype=np.int64))
    vals = rng.permutation(vals)[:d]
    assert len(vals) == d
    keys = np.concatenate([vals, rng.choice(vals, size=n - d)])
    return rng.permutation(keys)


def remap_cases():
    """{name: int64 keys}: n on the 256-thread block and on powers of two (pad keys of the
    second sort reach 2n - 1 = the top of bits_for(2n)), by distinct count."""
    cases = {}
    for n in (1, 2, 255, 256, 257, 1024, 1 << 16, (1 << 16) + 1):
        for kind, d in (("distinct", n), ("equal", 1), ("n-1", n - 1), ("half+1", 1 + n // 2)):
            if 1 <= d <= n:
                cases[f"n{n}-{kind}"] = keys_with_distinct(n, d, seed=n + d)
    cases["extremes"] = np.array([0, INT64_MAX, -1, INT64_MIN, -1, INT64_MAX, 0, INT64_MIN, 7],
                                 dtype=np.int64)
    cases["descending"] = np.tile(np.arange(299, -1, -1, dtype=np.int64) * 3 - 450, 2)
    ends = keys_with_distinct(513, 100, seed=3)
    ends[ends == ends[0]] = ends[1]
    ends[0] = ends[-1] = 12345678901
    cases["first-and-last"] = ends
    return cases


def corner_coo(n, n_rows, n_cols, seed):
    """n entries over the shape: (0, 0) twice and (n_rows-1, n_cols-1) three times when n allows,
    the rest random cells; a single entry is the top corner (the largest key)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=n)
    cols = rng.integers(0, n_cols, size=n)
    top = [n - 1, 0, n // 2] if n >= 5 else [n - 1]
    rows[top], cols[top] = n_rows - 1, n_cols - 1
    if n >= 5:
        rows[[1, n - 2]], cols[[1, n - 2]] = 0, 0
    return rows.astype(np.int32), cols.astype(np.int32)
