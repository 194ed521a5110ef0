"""Inputs and numpy restatements for the structure-primitive edge tests
(tests/test_gpu_structure_edges.py). No GPU code here: graphs with an exact entry count built from
a degree vector, the row layouts and keep-masks that sit on the guards of the tiled compaction
(2,048-entry tiles, 256-entry rounds, 64-lane waves, 256-thread blocks), and the two restatements
the oracle lacks — the fp32 edge-order row sum of ``hgd_degree_scale`` and the rebuilt-from-scratch
reference of ``Incidence.drop``. Everything else is ``oracle.hgd_oracle``.
"""
import numpy as np

from oracle import hgd_oracle as O

TILE = 2048   # entries per tile of the compaction (kTile, csrc/structure.hip)
ROUND = 256   # entries per ballot round inside a tile (kTileThreads)
BLOCK = 256   # threads per block of the per-row kernels (kBlock)


def split_count(rng, total, parts):
    """``parts`` non-negative integers that sum to exactly ``total`` (a multinomial draw)."""
    return rng.multinomial(int(total), np.full(parts, 1.0 / parts)).astype(np.int64)


def coo_from_degrees(rng, degs, n_cols, col_p=None):
    """Row-sorted COO with exactly ``degs[r]`` entries in row r, unique (row, col) pairs, the
    columns of every row ascending. ``col_p``: column probabilities (a skewed draw)."""
    degs = np.asarray(degs, dtype=np.int64)
    assert degs.min(initial=0) >= 0 and degs.max(initial=0) <= n_cols
    rows = np.repeat(np.arange(len(degs), dtype=np.int64), degs)
    parts = [np.sort(rng.choice(n_cols, size=int(k), replace=False, p=col_p)) for k in degs if k]
    cols = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    return rows, cols


def graph_exact(n, seed=0):
    """(rows, cols, vals, (R, C)): a sorted COO of exactly ``n`` unique entries over about n / 6
    rows with random degrees (some rows come out empty)."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    n_rows = n // 6 + 2
    degs = split_count(rng, n, n_rows)
    n_cols = max(int(degs.max()) + 3, 11)
    rows, cols = coo_from_degrees(rng, degs, n_cols)
    vals = (rng.random(n) + 0.5).astype(np.float32)
    return rows, cols, vals, (n_rows, n_cols)


LAYOUTS = ("leading_empty", "trailing_empty", "middle_empty", "row_at_tile", "one_row",
           "rows255", "rows256", "rows257")


def layout_degrees(name, n, rng):
    """The degree vector (sum exactly ``n``, n > TILE) of one named row layout."""
    if name == "leading_empty":
        return np.concatenate([np.zeros(5, np.int64), split_count(rng, n, 300)])
    if name == "trailing_empty":  # rowptr[r] == nnz for the last rows and for r == n_rows
        d = np.concatenate([split_count(rng, n - 1, 300), np.zeros(6, np.int64)])
        d[299] += 1
        return d
    if name == "middle_empty":
        return np.concatenate([split_count(rng, n // 2, 140), np.zeros(9, np.int64),
                               split_count(rng, n - n // 2, 150)])
    if name == "row_at_tile":  # a row starts exactly at entry TILE
        head = split_count(rng, TILE, 200)
        tail = split_count(rng, n - TILE - 1, 40)
        tail[0] += 1
        return np.concatenate([head, tail])
    if name == "one_row":
        return np.array([n], dtype=np.int64)
    if name.startswith("rows"):  # the r == n_rows thread is the last of a block / the first of one
        return split_count(rng, n, int(name[4:]))
    raise KeyError(name)


def graph_layout(name, n, seed=0):
    """(rows, cols, vals, (R, C)) of exactly ``n`` entries in the named row layout."""
    rng = np.random.default_rng(2000 + 13 * n + LAYOUTS.index(name) + seed)
    degs = layout_degrees(name, n, rng)
    assert degs.sum() == n and (degs >= 0).all()
    n_cols = max(int(degs.max()) + 5, 64)
    rows, cols = coo_from_degrees(rng, degs, n_cols)
    vals = (rng.random(n) + 0.5).astype(np.float32)
    return rows, cols, vals, (len(degs), n_cols)


MASKS = ("all", "none", "first", "last", "round_heads", "odd_tiles", "random")


def keep_mask(name, n, seed=0):
    """The named keep-mask over ``n`` entries (bool), or None where it does not apply
    (``odd_tiles`` needs more than one tile)."""
    e = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "first":
        return e == 0
    if name == "last":
        return e == n - 1
    if name == "round_heads":  # only the first entry of every 256-entry round
        return e % ROUND == 0
    if name == "odd_tiles":    # every entry of odd tiles, none of even tiles
        return (e // TILE) % 2 == 1 if n > TILE else None
    if name == "random":
        return O.device_keep_mask(seed + n, n, 0.5)
    raise KeyError(name)


def drop_reference(rows, cols, vals, keep, keep_rate, shape):
    """``Incidence.drop`` restated: the kept COO rebuilt from scratch. Returns a dict with
    ``rowptr, col, val, colptr, row_t, val_t, nnz`` (val / val_t None for a binary matrix); the
    kept values are ``vals[keep] / float32(keep_rate)`` in float32."""
    keep = np.asarray(keep, dtype=bool)
    R, C = shape
    v = None
    if vals is not None:
        v = (np.asarray(vals, np.float32)[keep] / np.float32(keep_rate)).astype(np.float32)
    rowptr, col, vv, _ = O.csr_from_coo(rows[keep], cols[keep], R, v)
    colptr, row_t, vt, _ = O.transpose_csr(rowptr, col, C, vv)
    return dict(rowptr=rowptr, col=col, val=vv, colptr=colptr, row_t=row_t, val_t=vt,
                nnz=int(keep.sum()))


def row_sums_f32(ptr, val):
    """Σ val over each row in float32, one addition per entry in entry order — the weighted
    degree of ``hgd_degree_scale`` (and of scipy's float32 row sum)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    val = np.asarray(val, dtype=np.float32)
    deg = np.diff(ptr)
    s = np.zeros(len(deg), dtype=np.float32)
    for k in range(int(deg.max(initial=0))):  # the k-th entry of every row that has one
        live = np.nonzero(deg > k)[0]
        s[live] = s[live] + val[ptr[live] + k]
    return s


def plan_degrees(n_rows, variant, rng):
    """Row degrees for the split-plan tests at threshold 16: ``mixed`` has light rows (0..16,
    some exactly 16) and heavy rows of 17, 24, 25 and 400 entries in the first wave, in the last
    wave of a block, in the last block and as the very last row; ``light`` has no heavy row;
    ``heavy`` has only heavy rows (17..40)."""
    if variant == "heavy":
        return rng.integers(17, 41, n_rows).astype(np.int64)
    d = rng.integers(0, 17, n_rows).astype(np.int64)
    d[[0, 2]] = 16
    if variant == "light":
        return d
    assert variant == "mixed"
    d[[1, 5, 40, 60]] = (17, 24, 25, 400)              # first wave of the first block
    for r, k in ((70, 17), (130, 25), (200, 24), (254, 17), (255, 25),  # later waves, block 0
                 (256, 24), (511, 17), (700, 400)):
        if r < n_rows:
            d[r] = k
            if r + 1 < n_rows:
                d[r + 1] = 16                          # exactly the threshold: not heavy
    d[n_rows - 2] = 25                                 # last block
    d[n_rows - 1] = 24                                 # the very last row
    return d
