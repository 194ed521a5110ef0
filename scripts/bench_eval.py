#!/usr/bin/env python3
"""Time the batched scoring + top-K evaluation (evaluation.rank_users) for every user of a
dataset-shaped graph, beside the reference's per-user CPU formulation (score row, mask rated
items, find_k_largest ordering via the closed form (scripts/refops); numba is not installed, so the
CPU figure is a numpy port, timed on a user sample and scaled). One JSON line per variant.

``--fused`` adds ``gpu_rank_users_fused`` (hgd_rank_topk: no score matrix) beside
``gpu_rank_users`` in the same process: both warmed up at the shape, then alternated for
``--rounds`` rounds (median, min and max reported); before timing, the fused lists of 256 sampled
users are checked against float64 scores (the run exits non-zero if the check fails). ``--preset``
picks a shape: ``yelp`` (31,668 × 38,048), ``large`` (65,536 × 1,000,000) or ``serving``
(64 × 1,000,000, timed with the segments chosen by shape and forced to 1). ``--only-fused`` skips
the unfused path and the CPU port (a profiler run of the fused kernels alone)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {"yelp": (31_668, 38_048, 1_170_000), "large": (65_536, 1_000_000, 2_600_000),
           "serving": (64, 1_000_000, 2_600)}
RTOL = 1e-5  # the project's fp32 bound: |got - ref_f64| <= RTOL·Σ|terms|


def check_fused(np, ue, ie, R, ids, sc, sample, k, mask=-10e8):
    """The tolerance-aware check of the fused lists for the sampled users (the first k item
    embeddings are zero, so no seed copy reaches a list): distinct ids, non-increasing scores,
    rated ids carry exactly -10e8, each listed score within RTOL·Σ|terms| of the float64 score
    of its id, every unlisted item at most the last listed score plus its own bound."""
    iec = ie.astype(np.float64)
    for r, u in enumerate(sample):
        s64 = iec @ ue[u].astype(np.float64)
        bound = RTOL * (np.abs(iec) @ np.abs(ue[u]).astype(np.float64))
        rated = R.indices[R.indptr[u]:R.indptr[u + 1]]
        s64[rated] = mask
        bound[rated] = 0.0
        li, ls = ids[r], sc[r].astype(np.float64)
        ok = (len(set(li.tolist())) == k and (np.diff(ls) <= 0).all()
              and (np.abs(ls - s64[li]) <= bound[li]).all())
        ok = ok and (sc[r][np.isin(li, rated)] == np.float32(mask)).all()
        rest = np.ones(len(s64), bool)
        rest[li] = False
        ok = ok and (s64[rest] <= ls[-1] + bound[rest]).all()
        if not ok:
            return f"user {int(u)} (sample row {r})"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS))
    ap.add_argument("--users", type=int, default=31_668)
    ap.add_argument("--items", type=int, default=38_048)
    ap.add_argument("--edges", type=int, default=1_170_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--cpu-sample", type=int, default=200)
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-check", action="store_true",
                    help="skip the fused correctness check (a profiler run after a checked one)")
    args = ap.parse_args()
    if args.preset:
        args.users, args.items, args.edges = PRESETS[args.preset]
    import numpy as np
    import scipy.sparse as sp
    import torch

    from hypergraph_diffusion_for_recommendation_amd.evaluation import rank_users, rated_csr
    import refops as O

    u, i = O.synthetic_incidence(args.users, args.items, args.edges, seed=0)
    R = sp.csr_matrix((np.ones(len(u), np.float32), (u, i)), shape=(args.users, args.items))
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    ue = torch.randn(args.users, args.dim, device=dev, generator=g)
    ie = torch.randn(args.items, args.dim, device=dev, generator=g)
    fused = args.fused or args.only_fused
    if fused:
        ie[:args.k] = 0.0  # no seed copy reaches a list: the check below can ask for distinct ids
    rated = rated_csr(R, dev)
    users = torch.arange(args.users)
    shape = {"users": args.users, "items": args.items, "dim": args.dim, "k": args.k}
    flop = 2 * args.users * args.items * args.dim

    variants = []
    if not args.only_fused:
        variants.append(("gpu_rank_users", {}, {"score_bytes_written": 4 * args.users * args.items}))
    if fused:
        variants.append(("gpu_rank_users_fused", {"fused": True}, {"segments": "auto"}))
        if args.users <= 64:  # the segmented case: the same rows on one workgroup per user block
            variants.append(("gpu_rank_users_fused", {"fused": True, "segments": 1},
                             {"segments": 1}))
    if fused and not args.no_check:
        rng = np.random.default_rng(0)
        sample = np.sort(rng.choice(args.users, size=min(256, args.users), replace=False))
        ids, sc = rank_users(ue, ie, torch.from_numpy(sample), rated, args.k, fused=True)
        bad = check_fused(np, ue.cpu().numpy(), ie.cpu().numpy(), R, ids.cpu().numpy(),
                          sc.cpu().numpy(), sample, args.k)
        print(json.dumps(dict(shape, variant="fused_check", sampled_users=len(sample),
                              ok=bad is None, first_failure=bad)), flush=True)
        if bad is not None:
            sys.exit(1)
    times = {n: [] for n in range(len(variants))}
    for _, kw, _ in variants:
        rank_users(ue, ie, users, rated, args.k, **kw)  # warm-up of each at the shape
    for _ in range(args.rounds):
        for n, (_, kw, _) in enumerate(variants):  # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, sc = rank_users(ue, ie, users, rated, args.k, **kw)
            ids.cpu()
            times[n].append(time.perf_counter() - t0)
    gpu_s = None
    for n, (name, _, extra) in enumerate(variants):
        ts = sorted(times[n])
        med = ts[len(ts) // 2]
        gpu_s = med if gpu_s is None else gpu_s
        print(json.dumps(dict(shape, variant=name, seconds_all_users=round(med, 5),
                              seconds_min=round(ts[0], 5), seconds_max=round(ts[-1], 5),
                              rounds=len(ts), users_per_s=round(args.users / med, 1),
                              algorithmic_flop=flop, tflops=round(flop / med / 1e12, 2),
                              **extra)), flush=True)
    if args.only_fused or args.cpu_sample <= 0:
        return
    uec, iec = ue.cpu().numpy(), ie.cpu().numpy()
    n = min(args.cpu_sample, args.users)
    t0 = time.perf_counter()
    for uu in range(n):
        cand = (uec[uu] @ iec.T).astype(np.float32)
        cand[R.indices[R.indptr[uu]:R.indptr[uu + 1]]] = -10e8
        O.topk_closed_form(args.k, cand)
    cpu_s = (time.perf_counter() - t0) / n * args.users
    print(json.dumps({"variant": "cpu_port_per_user", "users": args.users, "items": args.items,
                      "k": args.k, "seconds_all_users": round(cpu_s, 3),
                      "users_per_s": round(args.users / cpu_s, 1),
                      "sample_users": n, "threads": torch.get_num_threads()}))


if __name__ == "__main__":
    main()
