"""Inputs and a numpy model of the selection for the top-K edge tests
(tests/test_gpu_topk_edges.py). No GPU code here: the kernel's sort key restated in numpy, the
branch a row takes (``plan``), and row builders that sit on the guards of csrc/topk.hip — the
2,048-key threshold-bin capacity of the two-pass path and the 256-column compaction tiles of the
generic path. Every builder asserts the ``plan`` it was asked for, so a construction that misses
its branch fails where it is built. The expected lists are ``oracle.hgd_oracle.topk_closed_form``
(and the literal ``find_k_largest`` on short rows); tests/test_topk_ref.py checks this module on
the CPU.
"""
import numpy as np

from oracle import hgd_oracle as O

BIN_SHIFT = 21   # bin = the key's top 11 bits (kHistBins = 2048, csrc/topk.hip)
BIN_CAP = 2048   # kBinCap: a threshold bin of more keys takes the generic path
TILE = 256       # columns per compaction round of the generic path (kTopkBlock)
K_MAX = 256      # kTopkMax
LITERAL_MAX_COLS = 300  # find_k_largest (a Python loop) only on rows this short

# One bin of 2^21 floats, [1.0, 1.25): exponent 127, the two leading mantissa bits 00.
BIN_LO, BIN_HI = np.float32(1.0), np.float32(1.25)
TIE = np.float32(1.125)  # the tied threshold value of tie_row, inside that bin


def float_key(x):
    """The kernel's order-preserving uint32 key: -0.0 folded onto +0.0, then the sign bit set
    for a non-negative float and every bit flipped for a negative one."""
    x = np.ascontiguousarray(x, dtype=np.float32).copy()
    x[x == 0] = np.float32(0.0)
    u = x.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_bin(x):
    """Histogram bin of the two-pass path: the key's top 11 bits."""
    return (float_key(x) >> np.uint32(BIN_SHIFT)).astype(np.int64)


def plan(row, k):
    """(bin, need, in_bin, path): the bin holding the k-th largest key of ``row``, how many of
    its keys complete the k once every key of a higher bin is taken, its population, and the
    selection path the kernel takes for it ("two_pass", or "generic" above BIN_CAP keys)."""
    row = np.asarray(row, dtype=np.float32)
    assert 1 <= k <= len(row)
    hist = np.bincount(key_bin(row), minlength=1 << (32 - BIN_SHIFT))
    acc = 0
    for b in range(len(hist) - 1, -1, -1):
        if acc + hist[b] >= k:
            in_bin = int(hist[b])
            return b, k - acc, in_bin, "generic" if in_bin > BIN_CAP else "two_pass"
        acc += int(hist[b])
    raise AssertionError("unreachable: k <= len(row)")


def bits(x):
    """fp32 values as uint32 bit patterns (so -0.0 != +0.0 and every denormal counts)."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def expected(row, k):
    """(ids, score bits) the reference lists for one row: the closed form, cross-checked with
    the literal find_k_largest on short rows."""
    row = np.asarray(row, dtype=np.float32)
    ids, sc = O.topk_closed_form(k, row)
    if len(row) <= LITERAL_MAX_COLS:
        lit_ids, lit_sc = O.find_k_largest(k, row)
        assert ids == lit_ids, (k, ids[:8], lit_ids[:8])
        assert bits(np.asarray(sc, np.float32)).tolist() == \
            bits(np.asarray(lit_sc, np.float32)).tolist()
    return ids, bits(np.asarray(sc, dtype=np.float32))


def _in_bin_values(rng, count, lo=BIN_LO, hi=BIN_HI):
    """``count`` distinct fp32 values of [lo, hi), both inside the bin [1.0, 1.25)."""
    a, b = int(bits([lo])[0]), int(bits([hi])[0])
    assert count <= b - a
    off = rng.choice(b - a, size=count, replace=False).astype(np.uint32)
    return (off + np.uint32(a)).view(np.float32)


def bin_population(n_cols, k, in_bin, need, seed=0, clean_seeds=False):
    """One fp32 row whose threshold bin holds exactly ``in_bin`` keys of which ``need`` complete
    the top k: ``in_bin`` distinct values in [1.0, 1.25), ``k - need`` values at or above 1.25
    and the rest below 1.0, at shuffled positions. ``clean_seeds`` keeps the first k columns
    below 1.0: no seed copy then displaces the end of the list, so the list is the selection
    itself, down to the last key taken from the threshold bin."""
    assert 1 <= need <= min(in_bin, k) and in_bin + (k - need) <= n_cols
    rng = np.random.default_rng([n_cols, k, in_bin, need, seed])
    n_above = k - need
    n_below = n_cols - in_bin - n_above
    above = (BIN_HI + rng.integers(0, 64, size=n_above) * np.float32(0.25)).astype(np.float32)
    below = (rng.integers(-8, 8, size=n_below) * np.float32(0.125)).astype(np.float32)  # < 1.0
    row = np.concatenate([below, _in_bin_values(rng, in_bin), above]).astype(np.float32)
    if clean_seeds:
        assert n_below >= k
        row[k:] = row[k:][rng.permutation(n_cols - k)]
        assert (row[:k] < BIN_LO).all()
    else:
        row = row[rng.permutation(n_cols)]
    b, got_need, got_in_bin, path = plan(row, k)
    assert (b, got_need, got_in_bin) == (int(key_bin([BIN_LO])[0]), need, in_bin), \
        (b, got_need, got_in_bin)
    assert path == ("generic" if in_bin > BIN_CAP else "two_pass")
    return row


def tie_row(n_cols, k, tie_cols, n_above, in_bin=None, seed=0):
    """One fp32 row for the compaction guard: the threshold value TIE sits at exactly the
    columns ``tie_cols``, ``n_above`` columns hold larger values (at or above 1.25) and the first
    ``need = k - n_above`` ties in column order complete the k. ``in_bin`` (default: the ties
    alone) is the threshold bin's population: the difference is made up of distinct values of
    [1.0, TIE), which crowd the bin without tying. Every other column is below 1.0. Where the
    ties leave the first k columns free, the larger values do too: no seed copy then displaces
    the end of the list, and the ``need``-th tie is its last entry."""
    tie_cols = np.unique(np.asarray(tie_cols, dtype=np.int64))
    n_ties = len(tie_cols)
    in_bin = n_ties if in_bin is None else in_bin
    need = k - n_above
    assert 1 <= need <= n_ties <= in_bin and 0 <= n_above and in_bin + n_above <= n_cols
    assert tie_cols[0] >= 0 and tie_cols[-1] < n_cols
    rng = np.random.default_rng([n_cols, k, n_ties, n_above, in_bin, seed])
    free = np.setdiff1d(np.arange(n_cols), tie_cols)
    free = free[rng.permutation(len(free))]
    if tie_cols[0] >= k:  # larger values outside the seed window
        free = np.concatenate([free[free >= k], free[free < k]])
        assert n_above <= int((free >= k).sum())
    row = np.empty(n_cols, dtype=np.float32)
    row[tie_cols] = TIE
    above_cols, rest = free[:n_above], free[n_above:]
    rest = rest[rng.permutation(len(rest))]
    fill_cols, below_cols = rest[:in_bin - n_ties], rest[in_bin - n_ties:]
    row[above_cols] = BIN_HI + rng.integers(0, 64, size=n_above) * np.float32(0.25)
    row[fill_cols] = _in_bin_values(rng, len(fill_cols), BIN_LO, TIE)
    row[below_cols] = rng.integers(-8, 8, size=len(below_cols)) * np.float32(0.125)
    b, got_need, got_in_bin, path = plan(row, k)
    assert (b, got_need, got_in_bin) == (int(key_bin([TIE])[0]), need, in_bin)
    assert path == ("generic" if in_bin > BIN_CAP else "two_pass")
    assert np.array_equal(np.flatnonzero(row == TIE), tie_cols)
    assert int((row > TIE).sum()) == n_above
    assert tie_cols[0] < k or (row[:k] < TIE).all()
    return row


def nth_tie_at(n_cols, k, need, col, style, rng):
    """Tie columns, none of them among the first k (the seed window), whose ``need``-th in
    column order is ``col``; None where the style cannot hold that:
      "after"      need-1 ties scattered before ``col``, and every second later column a tie
                   that the selection must drop (None for the last column: nothing is later);
      "full_tile"  the whole 256-column tile of ``col`` is ties, the rest of the need before it
                   (None for a tile that overlaps the seed window, and unless ``need`` covers
                   the tile's columns up to ``col``);
      "late"       no tie in the first tile."""
    tile0 = col // TILE * TILE
    if style == "after":
        if col == n_cols - 1 or need - 1 > col - k:
            return None
        before = k + rng.choice(col - k, size=need - 1, replace=False)
        return np.concatenate([before, [col], np.arange(col + 2, n_cols, 2)])
    if style == "full_tile":
        in_tile = col - tile0 + 1  # ties of the tile up to and including col
        if tile0 < k or need < in_tile or need - in_tile > tile0 - k:
            return None
        before = k + rng.choice(max(tile0 - k, 1), size=need - in_tile, replace=False)
        return np.concatenate([before, np.arange(tile0, min(tile0 + TILE, n_cols))])
    if style == "late":
        lo = max(TILE, k)
        if col < lo or need - 1 > col - lo:
            return None
        before = lo + rng.choice(max(col - lo, 1), size=need - 1, replace=False)
        return np.concatenate([before, [col], np.arange(col + 1, n_cols, 3)])
    raise ValueError(style)


def mixed_rows(n_cols, k, rows=12, seed=0):
    """The content mix of tests/test_gpu_topk.py for any n_cols >= k: integer ties, top scores
    inside the seed window, normal draws, an all-equal row, a -0.0 among +0.0, rounded draws
    (crowded bins) and a half-masked row; and three rows whose lists name particular columns:
    ascending scores (the list is the last k columns, so a sweep that loses its tail shows),
    descending scores, and top scores at the columns where a sweep changes loop."""
    rng = np.random.default_rng([n_cols, k, seed])
    S = rng.integers(-6, 7, size=(rows, n_cols)).astype(np.float32)
    S[::3, :k] += 20.0
    S[1::4] = rng.standard_normal((len(S[1::4]), n_cols)).astype(np.float32)
    S[2, :] = 0.0
    S[2, n_cols // 2] = -0.0
    S[4] = np.arange(n_cols, dtype=np.float32) - n_cols // 2
    S[6] = np.round(rng.standard_normal(n_cols), 1).astype(np.float32)
    S[7, : n_cols // 2] = -10e8
    edges = [c for c in EDGE_COLS if c < n_cols] + [n_cols - 1 - j for j in range(min(5, n_cols))]
    edges = np.unique(edges)
    S[8, edges] = 100.0 + rng.permutation(len(edges))
    S[10] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), size=n_cols)
    S[11] = -np.arange(n_cols, dtype=np.float32)
    return S


# columns on either side of the sweeps' loop changes: one float4 per thread (column 1024), the
# unrolled body's four vectors per thread (4096, 8192) and their 256-vector strides in between
EDGE_COLS = (255, 256, 257, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 3071, 3072, 4092, 4093,
             4094, 4095, 4096, 4097, 4098, 8188, 8189, 8190, 8191, 8192)


# ---- the case tables shared by the CPU check of the builders and the GPU edge tests ----------
BIN_GUARD_IN_BIN = (1, 2047, 2048, 2049, 4096)
BIN_GUARD_K = (1, 40, 256)
BIN_GUARD_COLS = (6000, 6001)


def bin_guard_needs(in_bin, k):
    """need in {1, min(in_bin, k), k}, as far as a row can hold it: the bin cannot complete the
    k with more keys than it has, so need = k exists only where in_bin >= k."""
    return sorted({n for n in (1, min(in_bin, k), k) if n <= min(in_bin, k)})


def bin_guard_rows(n_cols, k, in_bin, rows=8):
    """``rows`` rows of one (n_cols, k, in_bin) cell, cycling through its ``need`` values; the
    second half with the seed window below the bin (the list is then the selection itself)."""
    needs = bin_guard_needs(in_bin, k)
    return np.stack([bin_population(n_cols, k, in_bin, needs[r % len(needs)], seed=r,
                                    clean_seeds=r >= rows // 2) for r in range(rows)])


COMPACTION_COLS = (255, 256, 257, 511, 512, -1)  # -1: the row's last column
COMPACTION_STYLES = ("after", "full_tile", "late")
COMPACTION_N_COLS = (2304, 2305, 4099)  # room for more than BIN_CAP keys in the threshold bin


def compaction_rows(n_cols, style, crowded=True):
    """[(k, col, row)]: for every guard column, one row per (need, k) in {(1, 1), (100, 137),
    (128, 128) or (256, 256)} that the style can hold there with the seed window free of ties;
    k = 137 puts 37 larger values ahead of the ties and is no power of two, the others are ties
    alone. ``crowded`` fills the threshold bin past BIN_CAP so the row takes the generic path;
    otherwise the bin holds the ties alone and the path follows their count."""
    rng = np.random.default_rng([n_cols, COMPACTION_STYLES.index(style), int(crowded)])
    out = []
    for col in COMPACTION_COLS:
        col = n_cols - 1 if col < 0 else col
        big = 256 if nth_tie_at(n_cols, 256, 256, col, style, rng) is not None else 128
        for need, n_above in ((1, 0), (100, 37), (big, 0)):
            k = need + n_above
            ties = nth_tie_at(n_cols, k, need, col, style, rng)
            if ties is None:
                continue
            n_ties = len(np.unique(ties))
            in_bin = max(n_ties, BIN_CAP + 1) if crowded else n_ties
            row = tie_row(n_cols, k, ties, n_above, in_bin=in_bin, seed=col)
            assert np.flatnonzero(row == TIE)[need - 1] == col and (row[:k] < TIE).all()
            out.append((k, col, row))
    return out


SPECIAL_KINDS = ("inf", "zero", "denormal", "masked")
MASK_VALUE = np.float32(-10e8)  # the reference's mark of a rated item


def special_rows(kind, n_cols, k, rows=8):
    """``rows`` fp32 rows of one family of special scores (n_cols >= k):
      "inf"       ±inf among finite scores: -inf over the whole seed window, rows of one
                  infinity alone, fewer than k finite scores (the threshold is -inf itself), more
                  +inf than k;
      "zero"      ±0.0 with fewer than k positive scores, so the threshold key is zero and the
                  listed zeros must keep the sign of their column;
      "denormal"  positive and negative denormals with ±0.0 between them;
      "masked"    all but max(k - 3, 0) columns hold -10e8, the others spread inside and outside
                  the seed window, so the list ends in masked items."""
    rng = np.random.default_rng([SPECIAL_KINDS.index(kind), n_cols, k])
    inf = np.float32(np.inf)
    S = np.empty((rows, n_cols), dtype=np.float32)
    for r in range(rows):
        if kind == "inf":
            x = rng.integers(-5, 6, size=n_cols).astype(np.float32) if r % 2 else \
                rng.standard_normal(n_cols).astype(np.float32)
            if r == 0:
                x[rng.random(n_cols) < 0.1] = inf
                x[rng.random(n_cols) < 0.1] = -inf
            elif r == 1:
                x[:k] = -inf
            elif r == 2:
                x[:] = -inf
            elif r == 3:
                x[:] = inf
            elif r == 4:  # fewer finite scores than k, one of them in the seed window
                keep = np.concatenate([[k // 2], k + rng.choice(n_cols - k, replace=False,
                                                               size=min(max(k - 4, 0), n_cols - k))])
                y = np.full(n_cols, -inf, dtype=np.float32)
                y[keep] = x[keep]
                x = y
            elif r == 5:
                x[: (k + 1) // 2] = inf
            elif r == 6:
                x[rng.random(n_cols) < 0.5] = -inf
            else:  # more +inf than k, some of them seeds
                x[rng.choice(n_cols, size=min(n_cols, k + 5), replace=False)] = inf
        elif kind == "zero":
            x = rng.choice(np.array([0.0, -0.0], np.float32), size=n_cols)
            n_pos = min(max(k - 3, 0), r)  # fewer than k positives: zeros complete the list
            n_neg = (n_cols - n_pos) // (r + 2)
            cols = rng.permutation(n_cols)
            x[cols[:n_pos]] = rng.integers(1, 4, size=n_pos)
            x[cols[n_pos:n_pos + n_neg]] = -rng.integers(1, 4, size=n_neg).astype(np.float32)
            if r == 6:
                x[x == 0] = np.float32(-0.0)
            if r == 7:
                x[:] = 0.0
                x[::5] = -0.0
        elif kind == "denormal":
            top = (5, 1 << 10, 1 << 21, (1 << 23) - 1)[r % 4]  # bit patterns below 2^23
            mag = rng.integers(1, top + 1, size=n_cols).astype(np.uint32)
            sign = (rng.random(n_cols) < 0.5).astype(np.uint32) << np.uint32(31)
            x = (mag | sign).view(np.float32).copy()
            zeros = rng.random(n_cols) < (0.5 if r < 4 else 0.9)
            x[zeros] = rng.choice(np.array([0.0, -0.0], np.float32), size=int(zeros.sum()))
        elif kind == "masked":
            x = np.full(n_cols, MASK_VALUE, dtype=np.float32)
            n_open = max(k - 3, 0)
            inside = min(n_open, r * k // (2 * rows))  # unmasked columns in the seed window
            cols = np.concatenate([rng.choice(k, size=inside, replace=False),
                                   k + rng.choice(n_cols - k, size=min(n_open - inside,
                                                                       n_cols - k), replace=False)])
            x[cols.astype(np.int64)] = rng.integers(-3, 4, size=len(cols))
        else:
            raise ValueError(kind)
        S[r] = x
    assert not np.isnan(S).any()
    return S


# ---- sweep forms: which loop of for_each_score a row takes -----------------------------------
SWEEP_K = 20
SWEEP_COLS = (SWEEP_K, SWEEP_K + 1, 255, 256, 257, 1023, 1024, 1025, 1027, 4093, 4095, 4096,
              4097, 4099, 8191, 8193)
SWEEP_LAYOUTS = ("contiguous", "ld+1", "ld+3", "ld_mult4", "offset1", "offset3")


def layout_geometry(name, n_cols):
    """(element offset of the first row inside its 16-byte aligned buffer, leading dimension) of
    a [rows, n_cols] view: contiguous, a column slice of a wider buffer (ld = n_cols + 1, + 3,
    the next multiple of 4 above n_cols), or a slice starting 1 or 3 columns in."""
    if name == "contiguous":
        return 0, n_cols
    if name in ("offset1", "offset3"):
        return int(name[-1]), n_cols + 4
    return 0, {"ld+1": n_cols + 1, "ld+3": n_cols + 3, "ld_mult4": (n_cols // 4 + 1) * 4}[name]


def sweep_forms(n_cols, off, ld, rows):
    """The loops of for_each_score that the rows of such a view run: "scalar" (the all-scalar
    sweep of a row that is not 16-byte aligned) or, for an aligned row, "unrolled" (the body of
    4 float4 per thread, from n_cols // 4 = 1024), "vector" (the per-thread float4 loop over
    what the unrolled body leaves) and "tail" (the n_cols % 4 last columns)."""
    forms = set()
    for r in range(rows):
        if (off + r * ld) % 4:
            forms.add("scalar")
            continue
        n4 = n_cols // 4
        if n4 >= 1024:
            forms.add("unrolled")
        if n4 % 1024:
            forms.add("vector")
        if n_cols % 4:
            forms.add("tail")
    return forms
