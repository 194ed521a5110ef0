#!/usr/bin/env python3
"""CPU model of how many gathers of a hop hit L2, by the order its rows are walked in (numpy
only; no GPU). The source of the model figures in DESIGN.md §4.1.

The model: a scaled copy of the bench graph (uniform users × uniform items, deduplicated) with
the L2 scaled by the same factor. Rows are walked in workgroups of 16 (one 16-lane group per row
at d = 64), the workgroups placed round-robin on 8 XCDs, each XCD walking its workgroups in
order and a row's gathers in edge order. A gather hits if the same XCD fetched the same source
row within its last `window` gathers: at full scale an XCD's 4 MiB of L2 holds 16,384 rows of
256 B, at --scale 0.1 the window is 1,638; a 512-B row (d = 128) halves it.

It prints the hit share in natural, in min-column and in the greedy shared-column order for the
hop into users, and for one source block of the hop into items (the rows of block 0 of --blocks,
in natural order, in ascending order of their first column in the block, ties in natural order,
empty pieces last, and in the block's greedy order). The greedy order is the library's own
(hgd_row_order_greedy / hgd_col_block_order_greedy, host code: libhgd.so must be built, no GPU is
used): placed, every XCD walking its own part cut into --chunks chunks, and for comparison the
same 8·chunks chunks as one sequence dealt round-robin like any other order. With --pool, beside
them the pooled greedy orders (hgd_row_order_greedy_pooled / hgd_col_block_order_greedy_pooled):
the XCDs that many at a time taking their rows in turn from one shared pool.

    python scripts/model_l2_order.py [--scale 0.1 --blocks 4 --window 1638 --chunks 1 --pool 1 8]
"""
import argparse
import os
import sys
import time

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


def _lib():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    return nat


def greedy_order(rowptr, col, n_cols, window, chunks=1, placed=True, col_cap=1024, threads=0):
    """The library's greedy order of the rows: placed on the XCDs (each walks its own part, cut
    into `chunks` chunks), or the same number of chunks as one unplaced sequence."""
    nat = _lib()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    order = np.empty(len(rowptr) - 1, dtype=np.int32)
    xcds, chunks = (XCDS, chunks) if placed else (1, XCDS * chunks)
    nat.check(nat.load().hgd_row_order_greedy(
        rowptr.ctypes.data, col.ctypes.data, len(order), n_cols, window, col_cap, ROWS_PER_WG,
        xcds, chunks, threads, order.ctypes.data), "hgd_row_order_greedy")
    return order


def greedy_block_orders(rowptr, col, n_cols, n_blocks, window, chunks=1, placed=True,
                        col_cap=1024, threads=0):
    """[n_blocks, n_rows]: the library's greedy order of every source block's rows."""
    nat = _lib()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    n = len(rowptr) - 1
    order = np.empty(n_blocks * n, dtype=np.int32)
    xcds, chunks = (XCDS, chunks) if placed else (1, XCDS * chunks)
    nat.check(nat.load().hgd_col_block_order_greedy(
        rowptr.ctypes.data, col.ctypes.data, n, n_cols, n_blocks, window, col_cap, ROWS_PER_WG,
        xcds, chunks, threads, order.ctypes.data), "hgd_col_block_order_greedy")
    return order.reshape(n_blocks, n)


def pooled_order(rowptr, col, n_cols, window, pool, col_cap=1024, threads=0):
    """The library's pooled greedy order of the rows: the XCDs `pool` at a time take their rows in
    turn from one shared pool (1: every XCD walks its own part, the placed order above)."""
    nat = _lib()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    order = np.empty(len(rowptr) - 1, dtype=np.int32)
    nat.check(nat.load().hgd_row_order_greedy_pooled(
        rowptr.ctypes.data, col.ctypes.data, len(order), n_cols, window, col_cap, ROWS_PER_WG,
        XCDS, pool, threads, order.ctypes.data), "hgd_row_order_greedy_pooled")
    return order


def pooled_block_orders(rowptr, col, n_cols, n_blocks, window, pool, col_cap=1024, threads=0):
    """[n_blocks, n_rows]: the library's pooled greedy order of every source block's rows."""
    nat = _lib()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    n = len(rowptr) - 1
    order = np.empty(n_blocks * n, dtype=np.int32)
    nat.check(nat.load().hgd_col_block_order_greedy_pooled(
        rowptr.ctypes.data, col.ctypes.data, n, n_cols, n_blocks, window, col_cap, ROWS_PER_WG,
        XCDS, pool, threads, order.ctypes.data), "hgd_col_block_order_greedy_pooled")
    return order.reshape(n_blocks, n)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=0.1,
                    help="share of the bench graph (10 M users × 1 M items × 100 M edges)")
    ap.add_argument("--blocks", type=int, default=4, help="source blocks of the hop into items")
    ap.add_argument("--window", type=int, default=None,
                    help="gathers an XCD's L2 remembers (default: 16384·scale; halve it for the "
                         "512-B rows of d = 128)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chunks", type=int, default=1,
                    help="chunks each XCD's part of the greedy order is cut into")
    ap.add_argument("--pool", type=int, nargs="*", choices=[1, 2, 4, 8], default=[],
                    help="also walk the pooled greedy orders of these widths (XCDs to a shared "
                         "pool; one chunk per part)")
    args = ap.parse_args()
    U, I, E = (int(round(n * args.scale)) for n in (10_000_000, 1_000_000, 100_000_000))
    window = args.window if args.window is not None else int(16384 * args.scale)
    rowptr, col = make_graph(U, I, E, args.seed)
    print(f"graph: {U} users x {I} items, {len(col)} edges; window {window} gathers per XCD")

    nat = hit_share(rowptr, col, np.arange(U), window)
    ordered = hit_share(rowptr, col, min_column_order(rowptr, col, I), window)
    print(f"into users: natural {100 * nat:.2f} %, min-column order {100 * ordered:.2f} %")
    t0 = time.perf_counter()
    placed = greedy_order(rowptr, col, I, window, args.chunks)
    build_s = time.perf_counter() - t0
    unplaced = greedy_order(rowptr, col, I, window, args.chunks, placed=False)
    print(f"into users: greedy order, {args.chunks} chunk(s) per XCD part: placed "
          f"{100 * hit_share(rowptr, col, placed, window):.2f} %, the same chunks unplaced "
          f"{100 * hit_share(rowptr, col, unplaced, window):.2f} % (built in {build_s:.2f} s)")

    for pool in args.pool:
        t0 = time.perf_counter()
        order = pooled_order(rowptr, col, I, window, pool)
        build_s = time.perf_counter() - t0
        print(f"into users: pooled greedy order, {pool} XCD(s) to a pool: "
              f"{100 * hit_share(rowptr, col, order, window):.2f} % (built in {build_s:.2f} s)")

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
    # (the library cuts the blocks at ⌊U·k / blocks⌋: block 0 is the same [0, U // blocks))
    placed = greedy_block_orders(cptr, crow, U, args.blocks, window, args.chunks)[0]
    unplaced = greedy_block_orders(cptr, crow, U, args.blocks, window, args.chunks,
                                   placed=False)[0]
    print(f"into items, one of {args.blocks} blocks: greedy order placed "
          f"{100 * hit_share(bptr, bcol, placed, window):.2f} %, unplaced "
          f"{100 * hit_share(bptr, bcol, unplaced, window):.2f} %")
    for pool in args.pool:
        t0 = time.perf_counter()
        order = pooled_block_orders(cptr, crow, U, args.blocks, window, pool)[0]
        build_s = time.perf_counter() - t0
        print(f"into items, one of {args.blocks} blocks: pooled greedy order, {pool} XCD(s) to a "
              f"pool: {100 * hit_share(bptr, bcol, order, window):.2f} % (all blocks built in "
              f"{build_s:.2f} s)")


if __name__ == "__main__":
    main()
