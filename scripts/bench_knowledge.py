#!/usr/bin/env python3
"""KG tables build on the GPU: ingest.KnowledgeGraph (hgd_kg_expand, the head sort, the
coalesce and the normalisation; host arrays in, synchronised device tables out) against the
NumPy / scipy restatement of Knowledge.construct_data + kg_interaction_mat + normalize_graph_mat
(tests/_unified_ref.py) on the same inputs, in interleaved rounds; median and range.

The restatement walks the table with one Python loop over plain lists; the reference walks the
same rows twice with DataFrame.iterrows(), which is slower still, so the restatement's time is a
lower bound on the reference's. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triples", type=int, default=1_000_000)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--users", type=int, default=30_000)
    ap.add_argument("--items", type=int, default=40_000)
    ap.add_argument("--entities", type=int, default=50_000)
    ap.add_argument("--relations", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    from hypergraph_diffusion_for_recommendation_amd import KnowledgeGraph
    from tests import _unified_ref as R

    rng = np.random.default_rng(0)
    users = rng.integers(0, args.users, args.records)
    items = rng.integers(0, args.items, args.records) + args.users
    training = np.stack([users, items, np.ones_like(users)], axis=1).astype(np.float64).tolist()
    h = rng.integers(args.users, args.users + args.items, args.triples)
    t = rng.integers(args.users, args.users + args.items + args.entities, args.triples)
    r = rng.integers(0, args.relations, args.triples)
    dev = torch.device("cuda")
    torch.zeros(1, device=dev)
    g = KnowledgeGraph(training, h, r, t, device=dev)  # warm-up: allocator, hipcub temp sizes
    torch.cuda.synchronize()
    nat, ref = [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        k = R.knowledge(training, h, r, t)
        R.normalize_graph_mat(R.kg_interaction_mat(k))
        ref.append(time.perf_counter() - t0)
        del k
        t0 = time.perf_counter()
        g = KnowledgeGraph(training, h, r, t, device=dev)
        torch.cuda.synchronize()
        nat.append(time.perf_counter() - t0)

    def stats(xs):
        return {"median_s": round(statistics.median(xs), 4), "min_s": round(min(xs), 4),
                "max_s": round(max(xs), 4)}
    print(json.dumps({"triples": args.triples, "records": args.records,
                      "n_kg_train": g.n_kg_train, "n_users_entities": g.n_users_entities,
                      "nnz_norm_kg_adj": int(g.norm_kg_adj.csr.col.numel()),
                      "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
                      "restatement": stats(ref), "knowledge_graph": stats(nat),
                      "speedup_median": round(statistics.median(ref) / statistics.median(nat), 1),
                      "speedup_worst_case": round(min(ref) / max(nat), 1)}), flush=True)


if __name__ == "__main__":
    main()
