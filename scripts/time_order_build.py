#!/usr/bin/env python3
"""Build time and peak memory of the greedy row orders on the host (numpy and libhgd.so only; no
GPU): hgd_row_order_greedy_pooled over the users' rows and hgd_col_block_order_greedy_pooled over
the items' rows in --blocks source blocks, at every --pool width, on a uniform graph the size of the
bench graph times --scale. A pool of 1 is the order of parts walked alone (hgd_row_order_greedy).
Every build runs in a process of its own, so that its peak resident set is its own; the graph is
made once and handed over as files.

    python scripts/time_order_build.py [--scale 1 --pool 1 8 --threads 0 --blocks 4]
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_l2_order as model  # noqa: E402


def child(args):
    nat = model._lib()
    lib = nat.load()
    rowptr = np.load(os.path.join(args.child, f"{args.form}_ptr.npy"))
    col = np.load(os.path.join(args.child, f"{args.form}_col.npy"))
    n, n_cols = len(rowptr) - 1, int(args.n_cols)
    # the resident set before and, sampled every 20 ms by a thread of its own, during the build
    # (the process's high-water mark may date from loading the graph)
    page = resource.getpagesize()

    def rss():
        with open("/proc/self/statm") as fh:
            return int(fh.read().split()[1]) * page

    base, peak, done = rss(), [0], threading.Event()

    def watch():
        while not done.wait(0.02):
            peak[0] = max(peak[0], rss())

    watcher = threading.Thread(target=watch, daemon=True)
    watcher.start()
    out = np.empty(max(1, args.blocks if args.form == "items" else 1) * n, dtype=np.int32)
    t0 = time.perf_counter()
    if args.form == "users":
        nat.check(lib.hgd_row_order_greedy_pooled(
            rowptr.ctypes.data, col.ctypes.data, n, n_cols, args.window, nat.ORDER_COL_CAP,
            model.ROWS_PER_WG, model.XCDS, args.pool[0], args.threads, out.ctypes.data), "users")
    else:
        nat.check(lib.hgd_col_block_order_greedy_pooled(
            rowptr.ctypes.data, col.ctypes.data, n, n_cols, args.blocks, args.window,
            nat.ORDER_COL_CAP, model.ROWS_PER_WG, model.XCDS, args.pool[0], args.threads,
            out.ctypes.data), "items")
    seconds = time.perf_counter() - t0
    done.set()
    watcher.join()
    print(json.dumps({"form": args.form, "pool": args.pool[0], "seconds": round(seconds, 2),
                      "rss_before_MiB": round(base / 2 ** 20),
                      "peak_rss_MiB": round(max(peak[0], base) / 2 ** 20)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--pool", type=int, nargs="+", default=[1, 8], choices=[1, 2, 4, 8])
    ap.add_argument("--threads", type=int, default=0,
                    help="0: the library's rule, min(work, OMP_NUM_THREADS if set, else 8)")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--window", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--form", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n-cols", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.window is None:
        args.window = max(1, int(16384 * args.scale))
    if args.child:
        return child(args)
    U, I, E = (int(round(n * args.scale)) for n in (10_000_000, 1_000_000, 100_000_000))
    print(f"OMP_NUM_THREADS {os.environ.get('OMP_NUM_THREADS', 'unset')} threads {args.threads} "
          f"cpus {os.cpu_count()}; {U} users x {I} items, window {args.window}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        rowptr, col = model.make_graph(U, I, E, args.seed)
        cptr, crow = model.transpose(rowptr, col, I)
        for name, a in (("users_ptr", rowptr), ("items_ptr", cptr)):
            np.save(os.path.join(tmp, name + ".npy"), a.astype(np.int64))
        for name, a in (("users_col", col), ("items_col", crow)):
            np.save(os.path.join(tmp, name + ".npy"), a.astype(np.int32))
        print(f"{len(col)} edges", flush=True)
        del rowptr, col, cptr, crow
        for form, n_cols in (("users", I), ("items", U)):
            for pool in args.pool:
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp,
                                "--form", form, "--n-cols", str(n_cols), "--pool", str(pool),
                                "--threads", str(args.threads), "--blocks", str(args.blocks),
                                "--window", str(args.window)], check=True)


if __name__ == "__main__":
    main()
