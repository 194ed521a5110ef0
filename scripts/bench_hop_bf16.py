#!/usr/bin/env python3
"""What does a bfloat16 embedding table buy the hop on MI355X? Per hop of hgconv2 (into items:
Hᵀ·X over the CSC, gathering the user table; into users: H·M over the CSR, gathering the item
table) this times the fp32 hop as the library runs it (source-blocked into items under the size
rule; HGD_SPMM_BLOCKS=0 in the environment makes it the plain hgd_spmm), the plain fp32 hop where
that differs, the bf16→bf16 hop (hgd_spmm_dt) and, where the structure allows blocking, the same
hop in --bf16-blocks source blocks (hgd_spmm_blocked_dt), on the same structure, weights and row
scales.

The variants alternate inside every round of one process (after untimed warm-up rounds); a
sample is --reps back-to-back launches between two device events. Reported per variant: median,
min and max ms per launch and TB/s on the variant's OWN algorithmic bytes
(profiling.hop_bytes with its element sizes); then the time ratio fp32 / bf16 next to the byte
ratio, which is its ceiling. One JSON line at the end.

    python scripts/bench_hop_bf16.py [--dim 64 --rounds 9 --zipf 1.0]
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
    ap.add_argument("--users", type=int, default=10_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds before the timed ones")
    ap.add_argument("--reps", type=int, default=5, help="launches per timed sample")
    ap.add_argument("--zipf", type=float, default=None,
                    help="item popularity exponent of bench.py's generator (default: uniform)")
    ap.add_argument("--pass-cols", type=int, default=0,
                    help="HGD_TUNE_SPMM_PASS_COLS for every variant (0 = the default passes)")
    ap.add_argument("--bf16-blocks", type=int, default=4,
                    help="source blocks of the blocked bf16 column (hgd_spmm_blocked_dt, timed "
                         "wherever the structure allows blocking; 0 = no such column)")
    args = ap.parse_args()

    import torch

    import bench
    from hypergraph_diffusion_for_recommendation_amd import Incidence, profiling
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_blocks, spmm_csr

    nat.check(nat.load().hgd_set_tuning(3, args.pass_cols), "pass cols")
    env_blocks = os.environ.get("HGD_SPMM_BLOCKS", "")  # ("" reads as unset: the size rule)
    dev = torch.device("cuda:0")
    U, I, d = args.users, args.items, args.dim
    idx = bench.make_graph(U, I, args.edges, 0, args.zipf, dev)
    inc = Incidence.from_coo(idx, None, (U, I), device=dev, validate=False, rows_sorted=True)
    del idx
    nnz = inc.nnz
    res = {"users": U, "items": I, "nnz": nnz, "dim": d, "zipf": args.zipf,
           "rounds": args.rounds, "reps": args.reps, "pass_cols": args.pass_cols,
           "HGD_SPMM_BLOCKS": os.environ.get("HGD_SPMM_BLOCKS", ""), "hops": {}}
    g = torch.Generator(device=dev).manual_seed(1)
    hops = {
        # name: (structure, source rows, output rows, per-nonzero weights, row scale)
        "into_items": (inc.csc, U, I, inc.edge_values("csc", "sym"), inc.scale("col", "mean")),
        "into_users": (inc.csr, I, U, None, inc.scale("row", "sym")),
    }
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for name, (S, n_src, R, w, q) in hops.items():
        X32 = torch.randn(n_src, d, device=dev, generator=g)
        X16 = X32.bfloat16()
        X32r = X16.float()  # the fp32 hop over the same (bf16-representable) values
        P = spmm_blocks(S, d)
        variants = {"fp32": (X32r, None, 4)}
        if P:  # the library blocks this hop: also time the plain one
            variants["fp32_plain"] = (X32r, 0, 4)
        variants["bf16"] = (X16, 0, 2)  # the plain hgd_spmm_dt, whatever the rule says
        os.environ["HGD_SPMM_BLOCKS"] = str(args.bf16_blocks)
        PB = spmm_blocks(S, d, torch.bfloat16) if args.bf16_blocks > 1 else 0
        os.environ["HGD_SPMM_BLOCKS"] = env_blocks
        if PB:  # the structure allows blocking: the bf16 hop in PB source blocks
            variants["bf16_blocked"] = (X16, PB, 2)

        def run(key):
            X, blocks, _ = variants[key]
            # spmm_csr takes None (the rule or the environment) or 0 (never): a count is forced
            # through the environment for that call
            os.environ["HGD_SPMM_BLOCKS"] = str(blocks) if blocks else env_blocks
            try:
                return spmm_csr(S, X, val=w, row_scale=q, blocks=None if blocks else blocks)
            finally:
                os.environ["HGD_SPMM_BLOCKS"] = env_blocks

        ref = run("fp32_plain" if P else "fp32")
        diff = float((run("bf16").float() - ref).abs().max() / ref.abs().max())
        del ref
        times = {k: [] for k in variants}
        for rnd in range(args.warmup + args.rounds):
            for key in variants:
                ev[0].record()
                for _ in range(args.reps):
                    Y = run(key)
                ev[1].record()
                torch.cuda.synchronize()
                del Y
                if rnd >= args.warmup:
                    times[key].append(ev[0].elapsed_time(ev[1]) / args.reps)
        out = {"fp32_blocks": P, "bf16_blocks": PB, "bf16_max_rel_diff_vs_fp32": diff,
               "variants": {}}
        for key, ts in times.items():
            eb = variants[key][2]
            nbytes = profiling.hop_bytes(nnz, R, d, x_bytes=eb, y_bytes=eb)
            ms = statistics.median(ts)
            out["variants"][key] = {"ms": round(ms, 4), "ms_min": round(min(ts), 4),
                                    "ms_max": round(max(ts), 4), "bytes_algorithmic": nbytes,
                                    "TBps_algorithmic": round(nbytes / ms / 1e9, 3)}
            print(f"{name:10s} {key:10s} {ms:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
                  f"{nbytes / 1e9:7.2f} GB  {nbytes / ms / 1e9:6.3f} TB/s", flush=True)
        v = out["variants"]
        out["time_ratio_fp32_over_bf16"] = round(v["fp32"]["ms"] / v["bf16"]["ms"], 3)
        out["byte_ratio_fp32_over_bf16"] = round(v["fp32"]["bytes_algorithmic"]
                                                 / v["bf16"]["bytes_algorithmic"], 3)
        print(f"{name:10s} time fp32/bf16 {out['time_ratio_fp32_over_bf16']:.3f}x  "
              f"(bytes {out['byte_ratio_fp32_over_bf16']:.3f}x)", flush=True)
        if PB:
            out["time_ratio_fp32_over_bf16_blocked"] = round(
                v["fp32"]["ms"] / v["bf16_blocked"]["ms"], 3)
            print(f"{name:10s} time fp32/bf16 blocked (P = {PB}) "
                  f"{out['time_ratio_fp32_over_bf16_blocked']:.3f}x", flush=True)
        res["hops"][name] = out
        del X32, X16, X32r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
