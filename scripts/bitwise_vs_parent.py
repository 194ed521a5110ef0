#!/usr/bin/env python3
"""Are two trees of this package the same function, bit for bit?

``dump --root TREE --out FILE`` imports the package from TREE (this checkout by default; a git
worktree of the parent commit, built the same way, for the other side), runs every hop operator
over seeded inputs and saves each result and gradient under a name. ``compare A B [--out TXT]``
loads two such files and prints one line per operator: how many tensors, and whether every one is
``torch.equal``; exit status 1 if any differs or a name is missing on either side.

Covered: spmm, two_hop (fp32, bf16 in / fp32 out, bf16 both ways), hgconv2, mean2hop,
att_two_hop, two_hop_fused and att_two_hop_fused (gather_dtype None / bfloat16, with and without
a caller's x16 and return_x16), spmm_csr_fused_dt (full and row range, with and without out16)
and the three KG encoders at two layers — over a 70 x 45 structure with one full row, with and
without forced split rows, weighted and unweighted, and as an edge-dropped masked view, at
d = 20, 64, 100, 320, slopes 0.2 and -0.1, and the pure blend (out_scale 0.7, Q None / mean).
Only names that exist in both trees are used."""
import argparse
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

N, M = 70, 45
WIDTHS = (20, 64, 100, 320)
SLOPES = (0.2, -0.1)
BF16, F32 = torch.bfloat16, torch.float32


def _coo(rng, n, m, nnz, full_row=None):
    key = rng.integers(0, n, nnz) * m + rng.integers(0, m, nnz)
    if full_row is not None:
        key = np.concatenate([key, full_row * m + np.arange(m)])
    key = np.unique(key)
    return key // m, key % m


def dump(root, out_path):
    sys.path.insert(0, root)
    pkg = importlib.import_module("hypergraph_diffusion_for_recommendation_amd")
    F = importlib.import_module(pkg.__name__ + ".functional")
    E = importlib.import_module(pkg.__name__ + ".encoders")
    nat = importlib.import_module(pkg.__name__ + "._native")
    assert os.path.realpath(os.path.dirname(pkg.__file__)).startswith(os.path.realpath(root))
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2024)
    out = {}

    def t(*shape, grad=False):
        a = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
        return a.requires_grad_(grad)

    def inc_of(r, c, vals, shape, split):
        kw = dict(split_threshold=32, split_chunk=16) if split else dict(split_threshold=0)
        idx = torch.from_numpy(np.stack([r, c]).astype(np.int64))
        v = None if vals is None else torch.from_numpy(np.asarray(vals, dtype=np.float32))
        return pkg.Incidence.from_coo(idx, v, shape, device=dev, **kw)

    def record(name, y, leaves, dY):
        """The outputs of one operator call and the gradient of every leaf."""
        ys = y if isinstance(y, tuple) else (y,)
        for k, v in enumerate(ys):
            out[f"{name}/y{k}"] = v.detach().cpu()
        leaves = [x for x in leaves if x is not None and x.requires_grad]
        grads = torch.autograd.grad(ys[0], leaves, dY.to(ys[0].dtype), allow_unused=True)
        for k, g in enumerate(grads):
            if g is not None:  # (γ and β of a call without LayerNorm)
                out[f"{name}/g{k}"] = g.cpu()

    r, c = _coo(rng, N, M, 600, full_row=7)
    w = rng.random(len(r)) + 0.1
    mask = torch.from_numpy(rng.random(len(r)) < 0.5)
    structures = {}
    for split in (False, True):
        for weighted in (True, False):
            name = ("w" if weighted else "u") + ("-split" if split else "")
            structures[name] = inc_of(r, c, w if weighted else None, (N, M), split)
    structures["masked"] = structures["w-split"].masked(mask, 0.5)
    ar, ac = _coo(rng, N, N, 400)
    aw = rng.random(len(ar)) + 0.1
    att = inc_of(ar, ac, aw / np.bincount(ar, weights=aw, minlength=N)[ar], (N, N), True)

    for sname, inc in structures.items():
        scaled = sname != "masked"  # (degree scales are the undropped structure's)
        PQR = dict(P="sym", Q="mean", R="sym") if scaled else {}
        for d in WIDTHS:
            X, res1, res2, dY = t(N, d, grad=True), t(N, d, grad=True), t(N, d, grad=True), t(N, d)
            XM, dYM = t(M, d, grad=True), t(M, d)
            norm = torch.nn.LayerNorm(d).to(dev)
            with torch.no_grad():
                norm.weight.copy_(torch.from_numpy(rng.random(d).astype(np.float32) + 0.5))
                norm.bias.copy_(t(d))
            params = [X, res1, res2, norm.weight, norm.bias]
            tag = f"{sname}/d{d}"
            record(f"spmm/{tag}", F.spmm(inc, XM), [XM], dY)
            record(f"spmm-t/{tag}", F.spmm(inc, X, transpose=True), [X], dYM)
            record(f"spmm-bf16/{tag}", F.spmm(inc, XM.bfloat16(), out_dtype=F32), [XM], dY)
            if scaled:
                record(f"hgconv2/{tag}", F.hgconv2(inc, X), [X], dY)
                record(f"mean2hop/{tag}", F.mean2hop(inc, X), [X], dY)
            X16 = X.detach().bfloat16()
            for slope in SLOPES:
                act = dict(epilogue="leaky_relu", slope=slope)
                st = f"{tag}/s{slope}"
                record(f"two_hop/{st}", F.two_hop(inc, X, **PQR, **act), [X], dY)
                record(f"two_hop-bf16-f32/{st}",
                       F.two_hop(inc, X.bfloat16(), **PQR, **act, out_dtype=F32), [X], dY)
                record(f"two_hop-bf16/{st}", F.two_hop(inc, X.bfloat16(), **PQR, **act), [X], dY)
                record(f"att_two_hop/{st}", F.att_two_hop(att, inc, X, **act), [X], dY)
                for ln in (True, False):
                    epi = dict(act, norm=norm if ln else None, out_scale=0.7, res1=res1,
                               res2=res2, res2_scale=0.3)
                    for gd in (None, BF16):
                        variants = [{}] if gd is None else [
                            dict(gather_dtype=gd, x16=x16, return_x16=rx)
                            for x16 in (None, X16) for rx in (False, True)]
                        for v in variants:
                            vt = (f"{st}/ln{int(ln)}/g{int(gd is not None)}"
                                  f"x{int(v.get('x16') is not None)}r{int(v.get('return_x16', 0))}")
                            record(f"two_hop_fused/{vt}",
                                   F.two_hop_fused(inc, X, **PQR, **epi, **v), params, dY)
                            record(f"att_two_hop_fused/{vt}",
                                   F.att_two_hop_fused(att, inc, X, **epi, **v), params, dY)
            # the pure blend: no LayerNorm, no activation, a pending out_scale in the backward
            for Q in ((None, "mean") if scaled else (None,)):
                for gd in (None, BF16):
                    v = {} if gd is None else dict(gather_dtype=gd)
                    bt = f"{tag}/blend/Q{Q}/g{int(gd is not None)}"
                    record(f"two_hop_fused/{bt}",
                           F.two_hop_fused(inc, X, Q=Q, out_scale=0.7, res1=res1, **v),
                           params[:2], dY)
                    record(f"att_two_hop_fused/{bt}",
                           F.att_two_hop_fused(att, inc, X, out_scale=0.7, res1=res1, **v),
                           params[:2], dY)
            # the fused bf16 hop by name: full and a row range, with and without the copy
            M16 = t(M, d).bfloat16()
            for ln in (True, False) if F._ln_supported16(d) else (False,):
                for rb, re_ in ((0, N), (10, 50)):
                    for copy16 in (False, True):
                        A = torch.zeros((N, d), device=dev)
                        stats = torch.zeros((N, 2), device=dev)
                        ex = nat.RowEpilogue(
                            act=nat.EPI_LEAKY_RELU, slope=0.2, layer_norm=int(ln), ln_eps=1e-5,
                            ln_gamma=norm.weight.data_ptr() if ln else None,
                            ln_beta=norm.bias.data_ptr() if ln else None, out_scale=0.7,
                            res1=res1.data_ptr(), ld_res1=d, res1_scale=1.0,
                            act_out=A.data_ptr(), ld_act=d,
                            stats=stats.data_ptr() if ln else None)
                        Y = torch.zeros((N, d), device=dev)
                        Y16 = torch.zeros((N, d), dtype=BF16, device=dev) if copy16 else None
                        pkg.spmm_csr_fused_dt(inc.csr, M16, ex, val=inc.val, out=Y, out16=Y16,
                                              row_begin=rb, row_end=re_)
                        ft = f"spmm_csr_fused_dt/{tag}/ln{int(ln)}/r{rb}-{re_}/c{int(copy16)}"
                        for k, v in (("y", Y), ("y16", Y16), ("act", A), ("stats", stats)):
                            if v is not None:
                                out[f"{ft}/{k}"] = v.cpu()

    # the encoders at two layers (the UGformer blocks in eval mode: no dropout draws)
    U, I, d, L = 40, 30, 64, 2
    u, i = _coo(rng, U, I, 300)
    wn = (rng.random(len(u)) + 0.1).astype(np.float32)
    n = U + I
    adj = inc_of(np.concatenate([u, i + U]), np.concatenate([i + U, u]), np.tile(wn, 2), (n, n),
                 False)
    kr, kc = _coo(rng, n, M, 500)
    kg = inc_of(kr, kc, rng.random(len(kr)) + 0.1, (n, M), False)
    kar, kac = _coo(rng, n, n, 300)
    kaw = rng.random(len(kar)) + 0.1
    katt = inc_of(kar, kac, kaw / np.bincount(kar, weights=kaw, minlength=n)[kar], (n, n), False)
    data = SimpleNamespace(n_users=U, n_items=I, norm_adj=None)
    x, wgt = t(n, d), t(n, d)
    torch.manual_seed(7)
    encoders = {
        "self": (E.SelfAwareEncoder(data, d, d, L, 0.2, 0.1, device=dev, use_self_att=False),
                 lambda e, z: torch.cat(e(z, adj))),
        "self-att": (E.SelfAwareEncoder(data, d, d, L, 0.2, 0.1, device=dev, use_self_att=True),
                     lambda e, z: torch.cat(e(z, adj))),
        "relational": (E.RelationalAwareEncoder(0.2, 0.1, L, d).to(dev),
                       lambda e, z: e(z, kg, None)),
        "khgrec": (E.KHGRecRelationalAwareEncoder(0.2, 0.1, L, d).to(dev),
                   lambda e, z: e(z, kg, katt)),
    }
    for name, (enc, call) in encoders.items():
        enc.eval()
        with torch.no_grad():
            for ln in enc.lns:
                ln.weight.uniform_(0.5, 1.5)
                ln.bias.uniform_(-0.2, 0.2)
        for gd in (None, BF16):
            enc.gather_dtype = gd
            for p in enc.parameters():
                p.grad = None
            xg = x.clone().requires_grad_(True)
            y = call(enc, xg)
            (y * wgt).sum().backward()
            et = f"encoder-{name}/g{int(gd is not None)}"
            out[f"{et}/y"] = y.detach().cpu()
            out[f"{et}/dx"] = xg.grad.cpu()
            for k, p in enumerate(enc.parameters()):
                if p.grad is not None:
                    out[f"{et}/p{k}"] = p.grad.cpu()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    torch.save(out, out_path)
    print(f"bitwise_vs_parent: {len(out)} tensors from {root} -> {out_path}", flush=True)


def compare(a_path, b_path, txt):
    a, b = torch.load(a_path), torch.load(b_path)
    per_op, bad = {}, []
    for name in sorted(set(a) | set(b)):
        op = name.split("/")[0]
        n_all, n_eq = per_op.get(op, (0, 0))
        same = (name in a and name in b and a[name].dtype == b[name].dtype
                and a[name].shape == b[name].shape
                and torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)))
        per_op[op] = (n_all + 1, n_eq + int(same))
        if not same:
            bad.append(name)
    lines = [f"{op}: {n_eq}/{n_all} tensors bitwise equal" for op, (n_all, n_eq) in per_op.items()]
    lines.append(f"total: {sum(v[1] for v in per_op.values())}/{sum(v[0] for v in per_op.values())}"
                 f" — {'EQUAL' if not bad else 'DIFFERENT: ' + ', '.join(bad[:20])}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if txt:
        os.makedirs(os.path.dirname(os.path.abspath(txt)), exist_ok=True)
        with open(txt, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    pd = sub.add_parser("dump")
    pd.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pd.add_argument("--out", required=True)
    pc = sub.add_parser("compare")
    pc.add_argument("a")
    pc.add_argument("b")
    pc.add_argument("--out")
    args = ap.parse_args()
    if args.cmd == "dump":
        dump(os.path.abspath(args.root), args.out)
    else:
        sys.exit(compare(args.a, args.b, args.out))
