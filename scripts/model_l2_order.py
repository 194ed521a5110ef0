#!/usr/bin/env python3
"""CPU model of how many gathers of a hop hit L2, by the order its rows are walked in (numpy
only; no GPU). The source of the model figures in DESIGN.md §4.1.

The model: a scaled copy of the bench graph (uniform users × uniform items, deduplicated) with
the L2 scaled by the same factor. Rows are walked in workgroups of 16 (one 16-lane group per row
at d = 64), the workgroups placed round-robin on 8 XCDs, each XCD walking its workgroups in
order and a row's gathers in edge order. A gather hits if the same XCD fetched the same source
row within its last `window` gathers: at full scale an XCD's 4 MiB of L2 holds 16,384 rows of
256 B, at --scale 0.1 the window is 1,638; a 512-B row (d = 128) halves it.

It prints the hit share in natural and in min-column order for the hop into users, and for one
source block of the hop into items (the rows of block 0 of --blocks, in natural order and in
ascending order of their first column in the block, ties in natural order, empty pieces last).

    python scripts/model_l2_order.py [--scale 0.1 --blocks 4 --window 1638]
"""
import argparse

import numpy as np

XCDS = 8
ROWS_PER_WG = 16


def make_graph(users, items, edges, seed):
    """(rowptr over users, item of every nonzero), rows sorted, columns ascending."""
    rng = np.random.default_rng(seed)
    key = np.unique(rng.integers(0, users, edges) * items + rng.integers(0, items, edges))
    u, i = key // items, key % items
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=users))])
    return rowptr, i


def transpose(rowptr, col, n_cols):
    """The CSC of a CSR with ascending columns: rows = the columns, their entries ascending."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))])
    return ptr, rows[order]


def hit_share(rowptr, col, order, window):
    """Share of the gathers that hit, walking the rows in `order`."""
    lens = np.diff(rowptr)[order]
    total = int(lens.sum())
    if total == 0:
        return 0.0
    # the gathers in walk order, and the XCD of each (its row's workgroup, round-robin)
    starts = rowptr[:-1][order]
    offs = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    stream = col[np.repeat(starts, lens) + offs]
    xcd = np.repeat((np.arange(len(order)) // ROWS_PER_WG) % XCDS, lens)
    hits = 0
    for x in range(XCDS):
        s = stream[xcd == x]
        # distance to the previous gather of the same source row on this XCD
        by_id = np.argsort(s, kind="stable")
        same = s[by_id][1:] == s[by_id][:-1]
        hits += int((np.diff(by_id)[same] <= window).sum())
    return hits / total


def min_column_order(rowptr, col, n_cols):
    """Rows in ascending order of their first (smallest) column; empty rows last; stable."""
    lens = np.diff(rowptr)
    key = np.full(len(lens), n_cols, dtype=np.int64)
    key[lens > 0] = col[rowptr[:-1][lens > 0]]
    return np.argsort(key, kind="stable")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=0.1,
                    help="share of the bench graph (10 M users × 1 M items × 100 M edges)")
    ap.add_argument("--blocks", type=int, default=4, help="source blocks of the hop into items")
    ap.add_argument("--window", type=int, default=None,
                    help="gathers an XCD's L2 remembers (default: 16384·scale; halve it for the "
                         "512-B rows of d = 128)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    U, I, E = (int(round(n * args.scale)) for n in (10_000_000, 1_000_000, 100_000_000))
    window = args.window if args.window is not None else int(16384 * args.scale)
    rowptr, col = make_graph(U, I, E, args.seed)
    print(f"graph: {U} users x {I} items, {len(col)} edges; window {window} gathers per XCD")

    nat = hit_share(rowptr, col, np.arange(U), window)
    ordered = hit_share(rowptr, col, min_column_order(rowptr, col, I), window)
    print(f"into users: natural {100 * nat:.2f} %, min-column order {100 * ordered:.2f} %")

    # block 0 of the hop into items: the CSC's entries among the first U/P users
    cptr, crow = transpose(rowptr, col, I)
    cut = U // args.blocks
    keep = crow < cut
    bptr = np.concatenate([[0], np.cumsum(keep)])[cptr]
    bcol = crow[keep]
    nat = hit_share(bptr, bcol, np.arange(I), window)
    order = min_column_order(bptr, bcol, cut)
    ordered = hit_share(bptr, bcol, order, window)
    print(f"into items, one of {args.blocks} blocks: natural {100 * nat:.2f} %, "
          f"block min-column order {100 * ordered:.2f} %")


if __name__ == "__main__":
    main()
