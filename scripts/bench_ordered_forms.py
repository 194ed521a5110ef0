#!/usr/bin/env python3
"""Does the structure's row order pay for the hops a model issues — the fused (LayerNorm +
residual), the edge-dropped (keep 0.5), the masked + fused and the bfloat16 forms of each? One
process; for every shape and form the order off (the unordered entry point) against on (its
ordered twin, HGD_SPMM_ROW_ORDER=1) in interleaved rounds of event-timed calls: the median of the
rounds' medians and the rounds' range, one JSON line per case. A form's rule
(hgd_spmm_row_order_for_dt) turns on only where on beat off by more than the rounds' ranges.

Shapes:
  bench64 / bench128   the bench graph's hop into users (10 M users x 1 M items x 100 M edges)
  local_aware          BASELINE configs[3]: LocalAwareEncoder, Amazon-Book shape, d = 128, fwd+bwd
  self_aware           the control: SelfAwareEncoder at the Yelp2018 shape, d = 64, fwd+bwd, where
                       the gathered table fits the aggregate L2 and the rule must stay off

A masked form's ordered call includes the view's own per-step cost, the byte gather of its mask
into the order's entry order (the cache on the view is cleared before every call); its share is
reported as mask_gather_ms. The orders and the ordered weights are built in the warm-up calls.

    python scripts/bench_ordered_forms.py [--shapes bench64,bench128,local_aware,self_aware]
        [--kind min|greedy] [--rounds 5] [--calls 10] [--users N --items N --edges N]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def measure(torch, run, rounds, calls):
    """{off, on}: the median of the rounds' medians, the rounds' range; interleaved rounds."""
    for on in (False, True):  # warm-up: the orders, the ordered weights, the allocator
        for _ in range(2):
            run(on)
    torch.cuda.synchronize()
    meds = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            ts = []
            for _ in range(calls):
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                run(on)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            meds[on].append(statistics.median(ts))
    out = {}
    for on, name in ((False, "off"), (True, "on")):
        out[name] = {"ms": round(statistics.median(meds[on]), 4),
                     "rounds_min_ms": round(min(meds[on]), 4),
                     "rounds_max_ms": round(max(meds[on]), 4)}
    out["on_over_off"] = round(out["on"]["ms"] / out["off"]["ms"], 4)
    spread = max(out[k]["rounds_max_ms"] - out[k]["rounds_min_ms"] for k in ("off", "on"))
    out["gain_ms"] = round(out["off"]["ms"] - out["on"]["ms"], 4)
    out["rounds_range_ms"] = round(spread, 4)
    # on beat off by more than the rounds' ranges: no overlap between the two sets of rounds
    out["on_wins"] = bool(out["on"]["rounds_max_ms"] < out["off"]["rounds_min_ms"]
                          and out["gain_ms"] > spread)
    return out


def set_order(on):
    os.environ["HGD_SPMM_ROW_ORDER"] = "1" if on else "0"


def hop_cases(torch, args, d, emit):
    import bench
    from hypergraph_diffusion_for_recommendation_amd import Incidence
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    from hypergraph_diffusion_for_recommendation_amd.incidence import (spmm_csr,
                                                                        spmm_csr_fused_dt,
                                                                        spmm_row_order)
    dev = torch.device("cuda:0")
    U0, I0, E0, _ = bench.WORKLOADS["synthetic"]
    U, I, E = args.users or U0, args.items or I0, args.edges or E0
    idx = bench.make_graph(U, I, E, 0, None, dev)
    inc = Incidence.from_coo(idx, None, (U, I), device=dev, rows_sorted=True).persist()
    del idx
    S = inc.csr
    g = torch.Generator(device=dev).manual_seed(d)
    X = torch.randn(I, d, device=dev, generator=g)
    X16 = X.bfloat16()
    res = torch.randn(U, d, device=dev, generator=g)
    gamma = torch.rand(d, device=dev, generator=g) + 0.5
    beta = torch.randn(d, device=dev, generator=g)
    q = inc.scale("row", "sym")
    mask = (torch.rand(S.nnz, device=dev, generator=g) < 0.5).to(torch.uint8)
    view = inc.masked(mask, 0.5).csr
    Y = torch.empty(U, d, device=dev)
    Y16 = torch.empty(U, d, device=dev, dtype=torch.bfloat16)
    A = torch.empty(U, d, device=dev)
    stats = torch.empty(U, 2, device=dev)
    ex = nat.RowEpilogue(act=nat.EPI_LEAKY_RELU, slope=0.2, layer_norm=1, ln_eps=1e-5,
                         ln_gamma=gamma.data_ptr(), ln_beta=beta.data_ptr(), out_scale=1.0,
                         res1=res.data_ptr(), ld_res1=d, res1_scale=1.0, act_out=A.data_ptr(),
                         ld_act=d, stats=stats.data_ptr())
    base = dict(shape=f"bench{d}", users=U, items=I, nnz=S.nnz, d=d, order_kind=args.kind,
                n_heavy=S.n_heavy)
    if S.n_heavy:
        emit(dict(base, skipped="split rows: no row order"))
        return
    os.environ.pop("HGD_SPMM_ROW_ORDER", None)

    def form(masked, fused, bf16):
        csr = view if masked else S
        os.environ.pop("HGD_SPMM_ROW_ORDER", None)  # (the rule, not what the last call forced)
        rule = bool(spmm_row_order(csr, d, torch.bfloat16 if bf16 else torch.float32,
                                   torch.bfloat16 if bf16 and not fused else torch.float32,
                                   fused, masked))

        def run(on):
            set_order(on)
            if masked:
                csr._mask_ord.clear()  # a view is made per step: its mask gather is per call
            if fused and bf16:
                return spmm_csr_fused_dt(csr, X16, ex, row_scale=q, out=Y, out16=Y16)
            if fused:
                return spmm_csr(csr, X, row_scale=q, out=Y, ex=ex)
            if bf16:
                return spmm_csr(csr, X16, row_scale=q, out=Y16, epilogue=nat.EPI_LEAKY_RELU,
                                slope=0.2)
            return spmm_csr(csr, X, row_scale=q, out=Y, epilogue=nat.EPI_LEAKY_RELU, slope=0.2)
        return rule, run

    for masked, fused in ((False, True), (True, False), (True, True), (False, False)):
        for bf16 in (False, True):
            if not masked and not fused and not bf16:
                continue  # the plain fp32 hop: scripts/bench_row_order.py
            name = ("masked_" if masked else "") + ("fused" if fused else "hop") + \
                ("_bf16" if bf16 else "")
            rule, run = form(masked, fused, bf16)
            want = [t.clone() for t in (run(False), A, stats, Y16)]
            got = [run(True), A, stats, Y16]
            same = all(torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else
                                          torch.int32),
                                   b.view(torch.int16 if b.dtype == torch.bfloat16 else
                                          torch.int32))
                       for a, b in zip(want, got)) if fused else torch.equal(want[0], got[0])
            del want, got
            rec = dict(base, form=name, rule=rule, bitwise_equal=bool(same))
            rec.update(measure(torch, run, args.rounds, args.calls))
            if masked:  # the view's own share of the ordered call
                perm = S._rows_of(None if args.kind == "min" else _geom(d, bf16, fused))[3]
                out = torch.empty_like(mask)
                lib = nat.load()

                def gather(on):
                    nat.check(lib.hgd_gather_u8(mask.data_ptr(), perm.data_ptr(), S.nnz,
                                                out.data_ptr(), nat.stream_handle(dev)), "g")
                rec["mask_gather_ms"] = measure(torch, gather, 3, args.calls)["on"]["ms"]
            emit(rec)


def _geom(d, bf16, fused):
    import torch

    from hypergraph_diffusion_for_recommendation_amd.incidence import order_geometry
    x = torch.bfloat16 if bf16 else torch.float32
    y = torch.bfloat16 if bf16 and not fused else torch.float32
    return order_geometry(d, False, x, y, fused)


def encoder_cases(torch, args, which, emit):
    import refops as R
    from hypergraph_diffusion_for_recommendation_amd import incidence as M
    from hypergraph_diffusion_for_recommendation_amd.encoders import (LocalAwareEncoder,
                                                                      SelfAwareEncoder)
    real_rule = M.spmm_row_order

    def parent_rule(csr, d, x_dtype=torch.float32, y_dtype=torch.float32, fused=False,
                    masked=False):
        if fused or masked or x_dtype != torch.float32 or y_dtype != torch.float32:
            return False
        return real_rule(csr, d)
    dev = torch.device("cuda")
    if which == "local_aware":
        U, I, E, d = 52_643, 91_599, 2_240_000, 128
    else:
        U, I, E, d = 31_668, 38_048, 1_237_259, 64
    u, i = R.synthetic_incidence(U, I, E, seed=0)
    ui = R.bipartite_adjacency(u, i, U, I).tocsr()
    data = types.SimpleNamespace(n_users=U, n_items=I, ui_adj=ui,
                                 norm_adj=R.normalize_graph_mat(ui).tocsr())
    torch.manual_seed(0)
    if which == "local_aware":
        enc = LocalAwareEncoder(data, d, d, 3, 0.3, 0.2, device=dev).train()
        adj = enc.sparse_norm_adj
    else:
        from hypergraph_diffusion_for_recommendation_amd.encoders import sparse_tensor_of
        enc = SelfAwareEncoder(data, d, d, 3, 0.1, 0.1, device=dev, use_self_att=False).train()
        adj = sparse_tensor_of(data.norm_adj, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    ego = torch.randn(U + I, d, device=dev, generator=g).requires_grad_(True)
    gout = torch.randn(U + I, d, device=dev, generator=g)
    modes = [("f32", None)]
    if hasattr(enc, "gather_dtype"):
        modes.append(("bf16", torch.bfloat16))
    for tag, gather in modes:
        if gather is not None:
            enc.gather_dtype = gather

        def run(on):
            # off is the parent commit's path: the plain fp32 hops by their size rule, every
            # other form unordered whatever its rule says by now
            if on:
                set_order(True)
                M.spmm_row_order = real_rule
            else:
                os.environ.pop("HGD_SPMM_ROW_ORDER", None)
                M.spmm_row_order = parent_rule
            enc.zero_grad(set_to_none=True)
            ego.grad = None
            ue, ie = enc(ego, adj)
            torch.autograd.backward([ue, ie], [gout[:U], gout[U:]])
            return torch.cat([ue.detach(), ie.detach()]), ego.grad

        outs = []
        for on in (False, True):  # (train mode: the same dropout draws both ways)
            torch.manual_seed(0)
            torch.cuda.manual_seed(0)
            outs.append([t.clone() for t in run(on)])
        (y0, g0), (y1, g1) = outs
        rec = dict(shape=which, form=f"fwd_bwd_{tag}", users=U, items=I, interactions=len(u), d=d,
                   order_kind="min", bitwise_equal=bool(torch.equal(y0, y1) and
                                                        torch.equal(g0, g1)))
        rec.update(measure(torch, run, args.rounds, args.calls))
        M.spmm_row_order = real_rule
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bench64,bench128,local_aware,self_aware")
    ap.add_argument("--kind", default="min", choices=("min", "greedy"),
                    help="the order the bench graph's hops walk: min column (built on the "
                         "device) or greedy shared-column (built on the host, once per geometry); "
                         "the encoders' structures do not persist and walk the min-column order")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--users", type=int, default=None)
    ap.add_argument("--items", type=int, default=None)
    ap.add_argument("--edges", type=int, default=None)
    args = ap.parse_args()
    if args.rounds < 5 or args.calls < 10:
        print("note: fewer than 5 rounds of 10 calls decides no rule", file=sys.stderr)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ordered_forms: needs a GPU; nothing is measured without one")
    os.environ["HGD_SPMM_ORDER_KIND"] = "1" if args.kind == "min" else "2"

    def emit(rec):
        print(json.dumps(rec), flush=True)

    for shape in args.shapes.split(","):
        if shape.startswith("bench"):
            hop_cases(torch, args, int(shape[5:]), emit)
        elif shape in ("local_aware", "self_aware"):
            encoder_cases(torch, args, shape, emit)
        else:
            raise SystemExit(f"unknown shape {shape!r}")
        torch.cuda.empty_cache()
    os.environ.pop("HGD_SPMM_ROW_ORDER", None)


if __name__ == "__main__":
    main()
