#!/usr/bin/env python3
"""Does blocking the into-items hop by USER range pay on MI355X? The hop Hᵀ·X gathers 256-B rows
of the 2.56 GB user table at random (5.9–6.4 TB/s, the random-gather ceiling), while the
into-users hop, whose 256 MB item table the 256 MB Infinity Cache (MALL) mostly holds, runs at
7.5 TB/s. Here the item hop is split into P phases, phase k summing only the neighbours in user
block k (a CSC of H's rows [u_k, u_k+1)), so each phase gathers from a U/P-row slice of X that
the MALL can hold; the phases accumulate into Y (Y = s·acc_k + Y). The price is P−1 extra
read+write passes over Y. Round 6 first emulated this with one sub-CSC per block and the fused
residual epilogue; it now times the library's hgd_spmm_blocked (one launch per block over the
block-major copy of the CSC, hgd_spmm_col_blocks, selected through HGD_SPMM_BLOCKS) against
hgd_spmm in interleaved rounds and reports the worst relative difference (a different fp32
summation order, so not bitwise).

--table-dtype bf16 times the same over a bfloat16 table (hgd_spmm_dt against hgd_spmm_blocked_dt;
--out-dtype: the output's type, default the table's): the same interleaved rounds, the median with
the min–max spread of the rounds, and TB/s on the variant's own algorithmic bytes
(profiling.hop_bytes with its element sizes).

--block-order on|both times the fp32 blocked hop over per-block row orders
(hgd_spmm_blocked_ordered over hgd_spmm_col_blocks_ordered, selected through
HGD_SPMM_BLOCK_ORDER) instead of, or interleaved with, hgd_spmm_blocked, and checks that the two
outputs are bitwise equal; with `both` the default block counts are 3,4,5,6, so that a shift of
the best P shows.

--packed both (with --block-order on|both) also times the ordered hop on packed entries
(hgd_spmm_blocked_packed, selected through HGD_SPMM_PACKED with the source scale stated) right
after each ordered variant, and checks that its output is bitwise the ordered hop's.

--zipf A draws the items ∝ rank^-A (bench.py's Zipf workload is A = 1): the CSC then has split
rows, the plain hop is hgd_spmm with its split plan, and the blocked variants are
hgd_spmm_blocked_split over a split plan per source block (selected through
HGD_SPMM_BLOCKS_SPLIT; HGD_SPMM_BLOCKS has no say on such a structure). --repeats N runs the
interleaved rounds N times in the same process and reports each.

    python scripts/bench_mall_blocked.py [--dim 64 --rounds 5 --table-dtype bf16]
    python scripts/bench_mall_blocked.py --zipf 1.0 --blocks 2,4,8 --repeats 2 [--dim 128]
    python scripts/bench_mall_blocked.py --block-order both [--dim 128 --blocks 6,8,10]
    python scripts/bench_mall_blocked.py --block-order on --packed both --blocks 4,5
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=1,
                    help="run the interleaved rounds this many times (one result line each)")
    ap.add_argument("--zipf", type=float, default=None,
                    help="items drawn ∝ rank^-A instead of uniformly: a CSC with split rows, "
                         "blocked as hgd_spmm_blocked_split (fp32 only)")
    ap.add_argument("--blocks", default=None,
                    help="block counts (default 2,4,8,10,16; 3,4,5,6 with --block-order both)")
    ap.add_argument("--block-order", choices=("off", "on", "both"), default="off",
                    help="each source block's rows in ascending order of their first column "
                         "(fp32 only): off, on, or both interleaved and compared bitwise")
    ap.add_argument("--packed", choices=("off", "both"), default="off",
                    help="both: every block-ordered variant also on packed entries (one word per "
                         "nonzero, no weight stream), interleaved and compared bitwise")
    ap.add_argument("--hop", choices=("items", "users"), default="items",
                    help="items: Hᵀ·X over the CSC (gathers the user table); users: H·M over the "
                         "CSR (gathers the item table)")
    ap.add_argument("--ld", type=int, default=0,
                    help="row stride of X (0 = dim): a column slice of a wider table, as the "
                         "sharded hop's 32-column slices of a d = 64 table")
    ap.add_argument("--unroll", type=int, default=8,
                    help="HGD_TUNE_SPMM_UNROLL for every variant (gathers in flight per lane)")
    ap.add_argument("--policy", type=int, default=8,
                    help="HGD_TUNE_SPMM_POLICY for every variant (8 = the default)")
    ap.add_argument("--seg", type=int, default=0,
                    help="HGD_TUNE_SPMM_BLOCKED_SEG for the blocked variants (1 = segmented walk)")
    ap.add_argument("--pass-cols", type=int, default=0,
                    help="HGD_TUNE_SPMM_PASS_COLS for every variant (0 = the default passes)")
    ap.add_argument("--table-dtype", choices=("f32", "bf16"), default="f32",
                    help="element type of the gathered table")
    ap.add_argument("--out-dtype", choices=("f32", "bf16"), default=None,
                    help="element type of the output (default: the table's)")
    args = ap.parse_args()

    import torch

    import bench
    from hypergraph_diffusion_for_recommendation_amd import Incidence, profiling
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_csr

    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    nat.check(nat.load().hgd_set_tuning(3, args.pass_cols), "pass cols")
    nat.check(nat.load().hgd_set_tuning(2, args.policy), "policy")
    nat.check(nat.load().hgd_set_tuning(1, args.unroll), "unroll")
    nat.check(nat.load().hgd_set_tuning(18, args.seg), "blocked seg")
    dev = torch.device("cuda:0")
    U, I, d = args.users, args.items, args.dim
    idx = bench.make_graph(U, I, args.edges, 0, args.zipf, dev)
    inc = Incidence.from_coo(idx, None, (U, I), device=dev, validate=False, rows_sorted=True)
    del idx
    nnz = inc.nnz
    if args.hop == "items":
        S, R = inc.csc, I
        X = torch.randn(U, max(d, args.ld), device=dev)[:, :d]
        q = inc.scale("col", "mean")
        w_full = inc.edge_values("csc", "sym")
        w_scale = inc.edge_src_scale("csc", "sym")
    else:
        # make_graph's COO is sorted by (user, item): every CSR row's columns ascend
        S, R = inc.csr, U
        rows = torch.repeat_interleave(torch.arange(U, device=dev), S.degrees())
        same = rows[1:] == rows[:-1]
        assert bool((S.col[1:][same] >= S.col[:-1][same]).all()), "CSR columns not ascending"
        del rows, same
        S.cols_ascending = True
        X = torch.randn(I, d, device=dev)
        q = inc.scale("row", "sym")
        w_full = w_scale = None
    dtypes = {"f32": torch.float32, "bf16": torch.bfloat16}
    x_dtype = dtypes[args.table_dtype]
    y_dtype = dtypes[args.out_dtype or args.table_dtype]
    if x_dtype != torch.float32:
        # (a column slice stays one: the wide table is converted, then cut again)
        X = X.to(x_dtype) if X._base is None else X._base.to(x_dtype)[:, :d]
    if args.block_order != "off" and (x_dtype, y_dtype) != (torch.float32, torch.float32):
        ap.error("--block-order needs an fp32 table and output")
    split = bool(S.n_heavy)  # split rows: the blocked variants are hgd_spmm_blocked_split
    if args.packed != "off" and (args.block_order == "off" or w_scale is None):
        ap.error("--packed needs --block-order on|both and the hop into items")
    if split and ((x_dtype, y_dtype) != (torch.float32, torch.float32)
                  or args.block_order != "off"):
        ap.error("a structure with split rows blocks only fp32 → fp32, without block orders")
    default_blocks = "3,4,5,6" if args.block_order == "both" else "2,4,8,10,16"
    counts = [int(p) for p in (args.blocks or default_blocks).split(",")]
    orders = {"off": ["0"], "on": ["1"], "both": ["0", "1"]}[args.block_order]
    # a variant: (P, HGD_SPMM_BLOCK_ORDER, HGD_SPMM_PACKED); its key in the output is P, P+ord with
    # the order, or P+ord+pk on packed entries
    blocks = [(P, o, pk) for P in counts for o in orders
              for pk in (["0", "1"] if o == "1" and args.packed == "both" else ["0"])]
    name = {(P, o, pk): (f"{P}+ord" + ("+pk" if pk == "1" else "")) if o == "1" else P
            for P, o, pk in blocks}
    for P, o, pk in blocks:  # block-major copies built outside the timed rounds
        if pk == "1":
            assert S.packed_entries(P, w_scale) is not None, "the hop does not fit the format"
        elif o == "1":
            S.col_blocks_ordered(P)
            S.blocked_ordered_values(P, w_full)
            S.blocked_ordered_scale(P, q)
        else:
            S.col_blocks(P)
            S.blocked_values(P, w_full)
            if split:
                S.col_block_plans(P)

    def run(P, order="0", packed="0"):
        # HGD_SPMM_BLOCKS=0: hgd_spmm; =P: hgd_spmm_blocked over P source ranges (spmm_blocks),
        # with HGD_SPMM_BLOCK_ORDER=1 hgd_spmm_blocked_ordered. Over a structure with split rows
        # HGD_SPMM_BLOCKS_SPLIT=0: hgd_spmm with its plan; =P: hgd_spmm_blocked_split
        os.environ["HGD_SPMM_BLOCKS"] = str(P)
        os.environ["HGD_SPMM_BLOCKS_SPLIT"] = str(P)
        os.environ["HGD_SPMM_BLOCK_ORDER"] = order
        os.environ["HGD_SPMM_PACKED"] = packed
        return spmm_csr(S, X, val=w_full, row_scale=q, out_dtype=y_dtype,
                        src_scale=w_scale if packed == "1" else None)

    ref = run(0).float()
    for rep in range(args.repeats):
        measure(args, run, ref, S, X, R, d, nnz, y_dtype, blocks, name, split, rep)


def measure(args, run, ref, S, X, R, d, nnz, y_dtype, blocks, name, split, rep):
    import torch

    from hypergraph_diffusion_for_recommendation_amd import profiling
    res = {"dim": d, "hop": args.hop, "pass_cols": args.pass_cols, "policy": args.policy, "unroll": args.unroll, "seg": args.seg, "ld": args.ld, "nnz": nnz,
           "table_dtype": args.table_dtype, "out_dtype": args.out_dtype or args.table_dtype,
           "rounds": args.rounds, "block_order": args.block_order, "packed": args.packed,
           "bytes_algorithmic": profiling.hop_bytes(nnz, R, d, x_bytes=X.element_size(),
                                                    y_bytes=4 if y_dtype == torch.float32 else 2),
           "zipf": args.zipf, "repeat": rep, "variants": {}}
    if split:
        # the plain hop's plan and each block count's plans: split rows and chunks (summed over
        # the blocks), and the share of the nonzeros the plain plan puts in split rows
        def total(P, field):
            return sum(int(getattr(p, field)) for p in S.col_block_plans(P))

        res["split"] = {"threshold": int(S.plan.threshold), "chunk": int(S.plan.chunk),
                        "n_heavy": int(S.plan.n_heavy), "n_chunks": int(S.plan.n_chunks),
                        "heavy_share": round(int(S.plan.n_chunks) * int(S.plan.chunk) / nnz, 4),
                        "blocks": {str(P): {"n_heavy": total(P, "n_heavy"),
                                            "n_chunks": total(P, "n_chunks")}
                                   for P, _, _ in blocks}}
    times = {"plain": []}
    times.update({name[v]: [] for v in blocks})
    diffs = {}
    bitwise = {}  # P -> the ordered hop's output equals hgd_spmm_blocked's bit for bit
    pk_bitwise = {}  # P -> the packed hop's output equals the ordered hop's bit for bit
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rnd in range(args.rounds + 1):
        kept = {}  # (first round, both) P -> hgd_spmm_blocked's output
        kept_ord = {}  # (first round, --packed both) P -> the ordered hop's output
        for v in ["plain"] + blocks:
            key = v if v == "plain" else name[v]
            ev[0].record()
            Y = run(0) if v == "plain" else run(*v)
            ev[1].record()
            torch.cuda.synchronize()
            if rnd:
                times[key].append(ev[0].elapsed_time(ev[1]))
            elif v != "plain":
                diffs[key] = float((Y.float() - ref).abs().max() / ref.abs().max())
                if v[2] == "1":
                    pk_bitwise[v[0]] = bool(torch.equal(Y, kept_ord.pop(v[0])))
                elif args.block_order == "both" and v[1] == "0":
                    kept[v[0]] = Y
                elif args.block_order == "both":
                    bitwise[v[0]] = bool(torch.equal(Y, kept.pop(v[0])))
                if v[1] == "1" and v[2] == "0" and args.packed == "both":
                    kept_ord[v[0]] = Y
            del Y
    if bitwise:
        res["ordered_bitwise_equal"] = {str(P): ok for P, ok in bitwise.items()}
        print("ordered output bitwise equal to hgd_spmm_blocked's:", bitwise, flush=True)
    if pk_bitwise:
        res["packed_bitwise_equal"] = {str(P): ok for P, ok in pk_bitwise.items()}
        print("packed output bitwise equal to hgd_spmm_blocked_ordered's:", pk_bitwise, flush=True)
    for key, ts in times.items():
        ms = statistics.median(ts)
        res["variants"][str(key)] = {"ms": round(ms, 4), "ms_min": round(min(ts), 4),
                                     "ms_max": round(max(ts), 4),
                                     "GBps_algorithmic": round(res["bytes_algorithmic"] / ms / 1e6,
                                                               1),
                                     "max_rel_diff_vs_plain": diffs.get(key, 0.0)}
        print(f"{str(key):6s} {ms:8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})  "
              f"{res['bytes_algorithmic'] / ms / 1e9:6.3f} TB/s", flush=True)
    print(json.dumps(res), flush=True)
    if not all(bitwise.values()):
        sys.exit("the ordered hop's output differs from hgd_spmm_blocked's")
    if not all(pk_bitwise.values()):
        sys.exit("the packed hop's output differs from hgd_spmm_blocked_ordered's")


if __name__ == "__main__":
    main()
