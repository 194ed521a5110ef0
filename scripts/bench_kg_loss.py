#!/usr/bin/env python3
"""KHGRec's per-minibatch TransR KG loss at the shape of conf/KHGRec.conf: B = 8192 triples,
d = 128, dr = 32; by default 100,000 entities and 40 relations, heads, tails and negative tails
drawn uniformly with replacement as util/sampler.py does. Forward + backward each:

    table        kg_loss on the embedding table with a prebuilt KGAttentionPattern (the step has
                 one for the attention anyway), validate=False: the gathers of KHGRec.py:124-126
                 are never materialised, dE is written whole
    table_nopat  the same without a pattern (the narrowing and the sort by r done here)
    rows         kg_loss_rows over three gathered [B, d] tensors (the gathers and their
                 index_put backward are torch's, as in the reference)
    index        the per-batch index work alone: narrowing the four id vectors, the sort by r
                 and its offsets, the 3B-key sort and row pointer of the scatter
    ref          the reference's ops with torch on the same GPU (refops.kg_loss_ref), the three
                 gathers from the table included

The variants run interleaved, --rounds rounds of --reps event-timed steps each; one JSON line
per variant with the median of the rounds' medians and the rounds' spread, and the peak device
memory one step adds (torch.cuda.max_memory_allocated over the step)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--relations", type=int, default=40)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rel-dim", type=int, default=32)
    ap.add_argument("--reg-kg", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variants (for a profiler pass)")
    args = ap.parse_args()
    import numpy as np
    import torch

    import refops as R
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import (KGAttentionPattern,
                                                                          _rowptr, _sort)
    from hypergraph_diffusion_for_recommendation_amd.kg_loss import (_narrow, kg_loss,
                                                                     kg_loss_rows, scatter_csr)

    if not torch.cuda.is_available():
        raise SystemExit("bench_kg_loss: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    n, nr, B, d, dr = args.entities, args.relations, args.batch, args.dim, args.rel_dim
    rng = np.random.default_rng(1)
    h, t, neg = (torch.from_numpy(rng.integers(0, n, B)).to(dev) for _ in range(3))
    r = torch.from_numpy(rng.integers(0, nr, B)).to(dev)
    torch.manual_seed(0)
    init = torch.nn.init.xavier_uniform_
    ego = torch.nn.Parameter(init(torch.empty(n, d)).to(dev))
    trans_M = torch.nn.Parameter(init(torch.empty(nr, d, dr)).to(dev))
    relation_emb = torch.nn.Parameter(init(torch.empty(nr, dr)).to(dev))
    params = (ego, trans_M, relation_emb)
    pattern0 = KGAttentionPattern(h, t, r, n, nr, validate=False)

    def clear():
        for p in params:
            p.grad = None

    def table():
        kg_loss(ego, h, t, neg, r, trans_M, relation_emb, args.reg_kg, B, pattern=pattern0,
                validate=False).backward()
        clear()

    def table_nopat():
        kg_loss(ego, h, t, neg, r, trans_M, relation_emb, args.reg_kg, B,
                validate=False).backward()
        clear()

    def rows():
        kg_loss_rows(ego[h], r, ego[t], ego[neg], trans_M, relation_emb, args.reg_kg, B,
                     validate=False).backward()
        clear()

    def index():
        flags = torch.zeros(1, dtype=torch.int64, device=dev)
        ids = [_narrow(x, n, flags, dev) for x in (h, t, neg)]
        r_sorted, _ = _sort(_narrow(r, nr, flags, dev), nr)
        _rowptr(r_sorted, nr)
        scatter_csr(torch.stack(ids).reshape(-1), n)

    def ref():
        R.kg_loss_ref(ego[h], r, ego[t], ego[neg], trans_M, relation_emb, args.reg_kg,
                      B).backward()
        clear()

    variants = [("table", table), ("table_nopat", table_nopat), ("rows", rows),
                ("index", index), ("ref", ref)]
    if args.only:
        variants = [v for v in variants if v[0] in args.only.split(",")]
    peak = {}
    for name, fn in variants:  # warm every shape, then one step's peak memory
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - before
    rounds = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            rounds[name].append(statistics.median(ts))
    for name, _ in variants:
        ms = rounds[name]
        print(json.dumps({"variant": name, "ms": round(statistics.median(ms), 4),
                          "ms_min_round": round(min(ms), 4), "ms_max_round": round(max(ms), 4),
                          "peak_extra_mb": round(peak[name] / 1e6, 2), "rounds": args.rounds,
                          "reps": args.reps, "entities": n, "relations": nr, "batch": B, "d": d,
                          "dr": dr}), flush=True)


if __name__ == "__main__":
    main()
