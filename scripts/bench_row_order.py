#!/usr/bin/env python3
"""Does walking the into-users hop's rows in min-column order pay on MI355X? The hop H·M gathers
~10 rows per user at random from the 256 MB item table, so an XCD's 4 MiB L2 sees no reuse; with
the rows processed in ascending order of their smallest column (hgd_spmm_row_order,
hgd_spmm_ordered, selected through HGD_SPMM_ROW_ORDER) the users sharing an item run next to
each other and the first gather of most rows can hit L2. The price is Y rows written in permuted
order. Times the hop with the order off and on in interleaved rounds (median), checks the two
outputs are bitwise equal, and prints one JSON line.

    python scripts/bench_row_order.py [--dim 64 --rounds 7 --workload synthetic|zipf --policy 8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic", choices=("synthetic", "zipf"))
    ap.add_argument("--users", type=int, default=None)
    ap.add_argument("--items", type=int, default=None)
    ap.add_argument("--edges", type=int, default=None)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--policy", type=int, default=8,
                    help="HGD_TUNE_SPMM_POLICY for both variants (8 = the default, 9 = with "
                         "non-temporal Y stores)")
    args = ap.parse_args()

    import torch

    import bench
    from hypergraph_diffusion_for_recommendation_amd import Incidence
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_csr, spmm_row_order

    nat.check(nat.load().hgd_set_tuning(2, args.policy), "policy")
    dev = torch.device("cuda:0")
    U0, I0, E0, zipf = bench.WORKLOADS[args.workload]
    U, I, E, d = args.users or U0, args.items or I0, args.edges or E0, args.dim
    idx = bench.make_graph(U, I, E, 0, zipf, dev)
    inc = Incidence.from_coo(idx, None, (U, I), device=dev, validate=False, rows_sorted=True)
    del idx
    S = inc.csr
    nnz = S.nnz
    os.environ.pop("HGD_SPMM_ROW_ORDER", None)
    rule = bool(spmm_row_order(S, d))
    X = torch.randn(I, d, device=dev)
    q = inc.scale("row", "sym")
    S.row_order()  # built outside the timed rounds, like the ordered row scale
    S.ordered_scale(q)

    def run(on):
        os.environ["HGD_SPMM_ROW_ORDER"] = "1" if on else "0"
        return spmm_csr(S, X, val=inc.val, row_scale=q)

    res = {"workload": args.workload, "users": U, "items": I, "dim": d, "nnz": nnz,
           "policy": args.policy, "rule": rule, "n_heavy": S.n_heavy,
           "bytes_algorithmic": nnz * (4 + 4 * d) + U * (4 * d + 4) + (U + 1) * 4}
    if S.n_heavy:  # split rows: the ordered hop does not apply
        print(json.dumps(res), flush=True)
        return
    ref = run(False)
    res["bitwise_equal"] = bool(torch.equal(run(True), ref))
    del ref
    times = {False: [], True: []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rnd in range(args.rounds + 1):
        for on in (False, True):
            ev[0].record()
            run(on)
            ev[1].record()
            torch.cuda.synchronize()
            if rnd:
                times[on].append(ev[0].elapsed_time(ev[1]))
    for on, name in ((False, "natural"), (True, "ordered")):
        ms = statistics.median(times[on])
        res[name] = {"ms": round(ms, 4), "min_ms": round(min(times[on]), 4),
                     "max_ms": round(max(times[on]), 4),
                     "GBps_algorithmic": round(res["bytes_algorithmic"] / ms / 1e6, 1)}
    res["ordered_over_natural"] = round(res["ordered"]["ms"] / res["natural"]["ms"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
