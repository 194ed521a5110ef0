#!/usr/bin/env python3
"""KHGRec's view fusion (KHGRec.py:132 / :202) at d = 128 over N = 100,000 and N = 1,000,000 rows:
the forward alone (evaluation, no_grad) and the forward with its backward (a training step; dOut
is a fixed tensor). Four contestants:

    fused        view_attention on the two separate views (hgd_view_attention_*); in training the
                 three parameters require a gradient, as the reference's module does
    fused_rows   (training only) the same with the parameters frozen: rows' gradients alone
    ref          the reference's ops with torch on the same GPU (refops.view_attention_ref), its
                 torch.stack included
    composed     the same expression from the library's existing functional.linear (the split-bf16
                 row GEMM) and torch element-wise ops: what the library could already do
    floor        a copy that moves the op's minimum bytes: 3·N·d·4 for the evaluation forward;
                 (4 + 6)·N·d·4 for the training forward (β0 saved) plus backward-data

The variants run interleaved, --rounds rounds of --reps event-timed steps each; one JSON line
per variant and size with the median of the rounds' medians and the rounds' spread, and the peak
device memory one step adds (torch.cuda.max_memory_allocated over the step)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variants (for a profiler pass)")
    args = ap.parse_args()
    import torch

    import refops as R
    from hypergraph_diffusion_for_recommendation_amd import view_attention
    from hypergraph_diffusion_for_recommendation_amd.functional import linear
    from hypergraph_diffusion_for_recommendation_amd.layers import Attention

    if not torch.cuda.is_available():
        raise SystemExit("bench_view_attention: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    d = args.dim
    for N in (int(x) for x in args.rows.split(",")):
        torch.manual_seed(0)
        init = torch.nn.init.xavier_uniform_
        z0 = init(torch.empty(N, d)).to(dev).requires_grad_(True)
        z1 = init(torch.empty(N, d)).to(dev).requires_grad_(True)
        g = torch.randn(N, d, device=dev)
        mod = Attention(d, d).to(dev)
        W1, b1, W2 = mod.weights()
        leaves = (z0, z1, W1, b1, W2)

        def clear():
            for p in leaves:
                p.grad = None

        def freeze(flag):
            for p in (W1, b1, W2):
                p.requires_grad_(not flag)

        def composed_expr():
            z = torch.stack([z0, z1], dim=1)
            t = torch.tanh(linear(z.reshape(2 * N, d), W1, b1))
            beta = torch.softmax(linear(t, W2).reshape(N, 2, d), dim=1)
            return (beta * z).sum(1)

        def train(expr):
            def step():
                expr().backward(g)
                clear()
            return step

        def evaluate(expr):
            def step():
                with torch.no_grad():
                    expr()
            return step

        def fused_rows():
            freeze(True)
            view_attention(z0, z1, W1, b1, W2).backward(g)
            freeze(False)
            clear()

        def floor(n_floats):
            src = torch.empty(n_floats // 2, device=dev)
            dst = torch.empty_like(src)
            return lambda: dst.copy_(src)

        fused = lambda: view_attention(z0, z1, W1, b1, W2)  # noqa: E731
        ref = lambda: R.view_attention_ref(torch.stack([z0, z1], dim=1), W1, b1, W2)[0]  # noqa: E731
        variants = [("eval_fused", evaluate(fused)), ("eval_ref", evaluate(ref)),
                    ("eval_composed", evaluate(composed_expr)), ("eval_floor", floor(3 * N * d)),
                    ("train_fused", train(fused)), ("train_fused_rows", fused_rows),
                    ("train_ref", train(ref)), ("train_composed", train(composed_expr)),
                    ("train_floor", floor(10 * N * d))]
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
                              "rounds": args.rounds, "reps": args.reps, "rows": N, "d": d}),
                  flush=True)
        del z0, z1, g, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
