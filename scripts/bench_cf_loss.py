#!/usr/bin/env python3
"""KHGRec's CF loss block (KHGRec.py:131-143) at B = 2,048, d = 128, 100,000 users over
n_items = 100,000 and 1,000,000: forward + backward into all leaves (the users, both item views
and the three Attention parameters). Variants:

    fused        cf_loss: the fusion at the batch's 2B positions only (hgd_cf_loss_*)
    fused_rows   the same with the parameters frozen: no parameter workspace, no split-K products
    composed     what the library could do before: view_attention over all items, bpr_loss_rows
                 and the regulariser in torch
    ref          the reference's ops with torch on the same GPU (refops.cf_loss_ref)

The variants run interleaved, --rounds rounds of --reps event-timed steps each; one JSON line per
variant and size with the median of the rounds' medians and the rounds' spread, the peak device
memory one step adds (torch.cuda.max_memory_allocated over the step), and the worst error of
`fused` and of `composed` on the timed inputs in units of the tests' bound: 1e-5 · mag against
the float64 restatement of tests/_cf_loss_ref64.py, evaluated on the CPU over the rows the batch
names (every other row of a table gradient must be exactly 0)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="100000,1000000")
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variants (for a profiler pass)")
    args = ap.parse_args()
    import torch

    import refops as R
    from hypergraph_diffusion_for_recommendation_amd import cf_loss, view_attention
    from hypergraph_diffusion_for_recommendation_amd.functional import bpr_loss_rows
    from hypergraph_diffusion_for_recommendation_amd.layers import Attention

    if not torch.cuda.is_available():
        raise SystemExit("bench_cf_loss: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    d, B, reg, bs = args.dim, args.batch, 0.01, args.batch
    for n_items in (int(x) for x in args.items.split(",")):
        torch.manual_seed(0)
        init = torch.nn.init.xavier_uniform_
        U = init(torch.empty(args.users, d)).to(dev).requires_grad_(True)
        z0 = init(torch.empty(n_items, d)).to(dev).requires_grad_(True)
        z1 = init(torch.empty(n_items, d)).to(dev).requires_grad_(True)
        mod = Attention(d, d).to(dev)
        W1, b1, W2 = mod.weights()
        leaves = (U, z0, z1, W1, b1, W2)
        uid = torch.randint(0, args.users, (B,), device=dev)
        pid = torch.randint(0, n_items, (B,), device=dev)
        nid = torch.randint(0, n_items, (B,), device=dev)

        def fused_expr():
            return cf_loss(U, z0, z1, uid, pid, nid, reg, bs, W1, b1, W2, validate=False)

        def composed_expr():
            fused = view_attention(z0, z1, W1, b1, W2)
            anc, pos, neg = U[uid], fused[pid], fused[nid]
            norms = torch.norm(anc, p=2) + torch.norm(pos, p=2) + torch.norm(neg, p=2)
            return bpr_loss_rows(U, fused, uid, pid, nid)[0] + norms * reg / bs

        def ref_expr():
            return R.cf_loss_ref(U, z0, z1, uid, pid, nid, reg, bs, W1, b1, W2)

        def train(expr, keep=False):
            def step():
                loss = expr()
                loss.backward()
                if keep:
                    return [loss.detach()] + [p.grad for p in leaves]
                for p in leaves:
                    p.grad = None
            return step

        def fused_rows():
            for p in (W1, b1, W2):
                p.requires_grad_(False)
            fused_expr().backward()
            for p in (W1, b1, W2):
                p.requires_grad_(True)
            for p in leaves:
                p.grad = None

        variants = [("fused", train(fused_expr)), ("fused_rows", fused_rows),
                    ("composed", train(composed_expr)), ("ref", train(ref_expr))]
        if args.only:
            variants = [v for v in variants if v[0] in args.only.split(",")]
        agree = {}
        if not args.only:  # outputs of fused and composed on the timed inputs
            from tests import _cf_loss_ref64 as T
            users, items = torch.unique(uid), torch.unique(torch.cat([pid, nid]))
            inp = dict(users=U[users], z0=z0[items], z1=z1[items], W1=W1, b1=b1, W2=W2,
                       uid=torch.searchsorted(users, uid), pid=torch.searchsorted(items, pid),
                       nid=torch.searchsorted(items, nid))
            ref, mag = T.reference({k: v.detach().cpu() for k, v in inp.items()}, reg, bs)
            rows = dict(dU=users, dZ0=items, dZ1=items)
            for name, expr in (("fused", fused_expr), ("composed", composed_expr)):
                got = dict(zip(("loss",) + T.GRADS, train(expr, keep=True)()))
                worst = 0.0
                for k, x in got.items():
                    if k in rows:  # nothing outside the batch's rows
                        assert int(torch.count_nonzero(x.abs().amax(1))) <= rows[k].numel(), k
                        x = x[rows[k]]
                    err = (x.detach().cpu().double() - ref[k]).abs()
                    assert bool((err[mag[k] == 0] == 0).all()), k
                    worst = max(worst, float((err / (1e-5 * mag[k] + 1e-300)).max()))
                agree[name] = worst
                for p in leaves:
                    p.grad = None
                del got
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
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                rounds[name].append(statistics.median(ts))
        for name, _ in variants:
            ms = rounds[name]
            print(json.dumps({"variant": name, "ms": round(statistics.median(ms), 4),
                              "ms_min_round": round(min(ms), 4),
                              "ms_max_round": round(max(ms), 4),
                              "peak_extra_mb": round(peak[name] / 1e6, 2),
                              "err_over_test_bound": agree.get(name),
                              "rounds": args.rounds,
                              "reps": args.reps, "batch": B, "users": args.users,
                              "items": n_items, "d": d}), flush=True)
        del U, z0, z1, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
