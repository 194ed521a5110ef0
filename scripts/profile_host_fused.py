#!/usr/bin/env python3
"""Host (Python) issue time of one layer's forward + backward for two_hop_fused, att_two_hop_fused
(each also with gather_dtype=torch.bfloat16) and hgconv2 on a graph so small (700 x 450, 6,000
nonzeros, d = 64) that the device never limits the loop: the minimum over 7 repeats of 1000 unsynchronised steps, one line per operator. It
resolves a few microseconds of Python per layer, which profile_host_overhead.py's single timing
at the ML-1M shape does not."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hypergraph_diffusion_for_recommendation_amd import Incidence  # noqa: E402
from hypergraph_diffusion_for_recommendation_amd import functional as F  # noqa: E402

dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
n, m, d = 700, 450, 64
key = np.unique(rng.integers(0, n, 6000) * m + rng.integers(0, m, 6000))
inc = Incidence.from_coo(torch.from_numpy(np.stack([key // m, key % m])), None, (n, m), device=dev)
ka = np.unique(rng.integers(0, n, 4000) * n + rng.integers(0, n, 4000))
att = Incidence.from_coo(torch.from_numpy(np.stack([ka // n, ka % n])),
                         torch.rand(len(ka)), (n, n), device=dev)
X = torch.randn(n, d, device=dev, requires_grad=True)
res = torch.randn(n, d, device=dev, requires_grad=True)
dY = torch.randn(n, d, device=dev)
norm = torch.nn.LayerNorm(d).to(dev)
leaves = [X, res, norm.weight, norm.bias]


def fused():
    Y = F.two_hop_fused(inc, X, P="sym", Q="mean", R="sym", epilogue="leaky_relu", slope=0.1,
                        norm=norm, res1=res)
    torch.autograd.grad(Y, leaves, dY)


def att_fused():
    Y = F.att_two_hop_fused(att, inc, X, epilogue="leaky_relu", slope=0.1, norm=norm, res1=res)
    torch.autograd.grad(Y, leaves, dY)


def fused16():
    Y = F.two_hop_fused(inc, X, P="sym", Q="mean", R="sym", epilogue="leaky_relu", slope=0.1,
                        norm=norm, res1=res, gather_dtype=torch.bfloat16)
    torch.autograd.grad(Y, leaves, dY)


def att_fused16():
    Y = F.att_two_hop_fused(att, inc, X, epilogue="leaky_relu", slope=0.1, norm=norm, res1=res,
                            gather_dtype=torch.bfloat16)
    torch.autograd.grad(Y, leaves, dY)


def plain():
    torch.autograd.grad(F.hgconv2(inc, X), X, dY)


for name, fn in (("two_hop_fused", fused), ("att_two_hop_fused", att_fused), ("hgconv2", plain),
                 ("two_hop_fused bf16", fused16), ("att_two_hop_fused bf16", att_fused16)):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(1000):
            fn()
        best = min(best, (time.perf_counter() - t0) / 1000)
        torch.cuda.synchronize()
    print(f"host_fused {name}: {1e6 * best:.2f} us/step (fwd+bwd, host issue, min of 7x1000)",
          flush=True)
