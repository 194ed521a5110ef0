#!/usr/bin/env python3
"""KHGRec's per-minibatch KG attention at the shape of conf/KHGRec.conf: B = 8192 triples,
d = 128, dr = 32, 2 layers; by default 100,000 entities, 40 relations and a KG adjacency of
1,000,000 nonzeros (10 per entity), heads and tails drawn uniformly with replacement as
util/sampler.py does.

(a) the attention update alone:
    update        KGAttentionPattern.update on a pattern built before (two launches + a gather)
    pattern       building the pattern (validate=False): the sorts, once per batch
    update_ref    the reference's update_attention with torch on the same GPU (refops), its
                  .cpu() softmax round trip included
(b) the KG encoder's forward + backward with a fresh attention per step:
    encoder       pattern + update + KHGRecRelationalAwareEncoder (four hops per layer)
    encoder_filt  the same with a `relations` filter that disables every fourth relation (the
                  disabled triples stay in the arrays, behind the last row)
    encoder_ref   update_attention + RelationalAwareEncoder with torch.sparse.mm(att, K) and the
                  two hops per layer, F.leaky_relu, F.layer_norm, add

The variants run interleaved, --rounds rounds of --reps event-timed steps each; one JSON line
per variant with the median of the rounds' medians and the rounds' spread."""
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
    ap.add_argument("--kg-edges", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rel-dim", type=int, default=32)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    import refops as R
    from hypergraph_diffusion_for_recommendation_amd.encoders import (
        KHGRecRelationalAwareEncoder, sparse_tensor_of)
    from hypergraph_diffusion_for_recommendation_amd.kg_attention import (KGAttentionPattern,
                                                                          relation_mask)

    if not torch.cuda.is_available():
        raise SystemExit("bench_kg_attention: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda")
    n, nr, B, d, dr, L = (args.entities, args.relations, args.batch, args.dim, args.rel_dim,
                          args.layers)
    u, v = R.synthetic_incidence(n, n, args.kg_edges, seed=0)
    import scipy.sparse as sp
    kg = sp.csr_matrix((np.ones(len(u), np.float32), (u, v)), shape=(n, n))
    kg_adj = sparse_tensor_of(R.normalize_graph_mat(kg), dev)  # norm_kg_adj, Incidence cached
    kg_ref = kg_adj.detach().clone().coalesce()
    rng = np.random.default_rng(1)
    h = torch.from_numpy(rng.integers(0, n, B)).to(dev)
    t = torch.from_numpy(rng.integers(0, n, B)).to(dev)
    r = torch.from_numpy(rng.integers(0, nr, B)).to(dev)
    relations = list(range(nr))
    torch.manual_seed(0)
    init = torch.nn.init.xavier_uniform_
    ego = torch.nn.Parameter(init(torch.empty(n, d)).to(dev))
    trans_M = init(torch.empty(nr, d, dr)).to(dev)
    relation_emb = init(torch.empty(nr, dr)).to(dev)
    dY = torch.randn(n, d, device=dev)
    enc = KHGRecRelationalAwareEncoder(0.2, 0.1, L, d).to(dev).train()
    pattern0 = KGAttentionPattern(h, t, r, n, nr, validate=False)

    def update():
        pattern0.update(ego, trans_M, relation_emb)

    def pattern():
        KGAttentionPattern(h, t, r, n, nr, validate=False)

    def update_ref():
        with torch.no_grad():
            R.update_attention(ego, h, t, r, relations, trans_M, relation_emb, (n, n))

    def encoder():
        att = KGAttentionPattern(h, t, r, n, nr, validate=False).update(ego, trans_M,
                                                                        relation_emb)
        enc(ego, kg_adj, att).backward(dY)
        ego.grad = None

    some = relation_mask([q for q in relations if q % 4], nr, dev)

    def encoder_filt():
        att = KGAttentionPattern(h, t, r, n, nr, some, validate=False).update(
            ego, trans_M, relation_emb)
        enc(ego, kg_adj, att).backward(dY)
        ego.grad = None

    def encoder_ref():
        with torch.no_grad():
            att = R.update_attention(ego, h, t, r, relations, trans_M, relation_emb, (n, n))
        x = ego
        for k in range(L):
            z = R.att_hgcn_conv(kg_ref, att, x, act=k != L - 1, slope=0.2)
            ln = enc.lns[k]
            x = F.layer_norm(z, (d,), ln.weight, ln.bias, ln.eps) + ego
        x.backward(dY)
        ego.grad = None

    variants = [("update", update), ("pattern", pattern), ("update_ref", update_ref),
                ("encoder", encoder), ("encoder_filt", encoder_filt),
                ("encoder_ref", encoder_ref)]
    for name, fn in list(variants):  # warm every shape
        try:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
        except (RuntimeError, NotImplementedError) as e:  # an op this torch build lacks
            if not name.endswith("_ref"):
                raise
            print(json.dumps({"variant": name, "error": str(e).splitlines()[0][:200]}),
                  flush=True)
            variants.remove((name, fn))
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
                          "rounds": args.rounds, "reps": args.reps, "entities": n,
                          "relations": nr, "kg_nnz": int(kg_ref._nnz()), "batch": B, "d": d,
                          "dr": dr, "layers": L}), flush=True)


if __name__ == "__main__":
    main()
