#!/usr/bin/env python3
"""Benchmark of the hot path: hypergraph-conv fwd+bwd M-edges/s at emb_dim=64, % HBM roofline.

A step is one forward + backward of the HGNN-normalised 2-hop conv
``Y = D_v^-1/2·H·D_e^-1·Hᵀ·D_v^-1/2·X`` (data/graph.py:28-42 of the reference) over one
synthetic user×item incidence H, i.e. four hgd_spmm hops: CSC (into items) + CSR (into users)
forward, the same pair backward. Unit of work = one nonzero of H.

    python bench.py [--gpus N --steps K --warmup W --workload synthetic|zipf|ml1m|yelp|amazon
                     --dim 64|256 --scaling strong|weak --full --dump-outputs DIR]

A plain run (``--gpus 1 --steps K --warmup W``) does only what the headline figure needs: it
builds the graph and the tables, warms up, times the K steps (``ms_per_step`` = the timed
region's wall time / K), writes the last timed step's outputs if ``--dump-outputs DIR`` is given,
and prints the result line. Everything below that takes runs of its own at N = 1 — the rocprofv3
PMC passes (``roofline.traffic``), the stream-copy peak (``roofline.measured_copy_*``), the CPU
reference with its ``parity`` gate and the ``cpu_baseline`` — runs only with ``--full`` (an
explicit ``--pmc on`` still collects the counters without it).

``--dump-outputs DIR`` writes what the last timed step returned, ``DIR/Y.npy`` and ``DIR/dX.npy``
(float32; ``_rank<r>`` is appended to the names at N > 1): all rows, or, above the size budget, a
fixed sample of rows (numpy generator seed 0, ascending) — the same rows in every run. Graph,
X and dY come from seeded generators, so two builds run with the same arguments can be compared
output for output.

N > 1 runs one process per GPU (RCCL over xGMI). Launched without WORLD_SIZE in the environment,
``--gpus N`` starts the N ranks itself (a child ``torch.distributed.run``, before this process
touches the GPU) and exits with its status; under a launcher WORLD_SIZE must equal --gpus.

* ``--scaling strong`` (default; BASELINE configs[4]): every rank builds the SAME global graph
  (seed 0) and keeps its degree-balanced user range (sharded.shard_rows_of_sorted_coo); value =
  global nonzeros × steps / max-over-ranks time. The item messages of every hop are all-reduced
  over xGMI in column slices pipelined with the hops (sharded.py).
* ``--scaling weak``: every rank owns its own full-size graph (seed = rank); value = Σ nonzeros.

Rank 0 prints ONE JSON line. ``roofline`` prices the dominant kernel (hgd_spmm) from HIP events
recorded around every hop launch on its stream during the timed steps, with SURVEY.md §8d's
algorithmic bytes. At N = 1 with ``--full`` the reference's own library calls (torch.sparse.mm + autograd on CPU,
oracle/ref_cpu.py) run once on the FULL graph and tables of the GPU run (copied to the host):
``parity`` compares one more GPU step with them row by row (the 1e-5 row bound; the script exits
non-zero if it fails), and ``cpu_baseline`` times the same calls on a bounded prefix sample of
the graph (median of 5 after 2 warm-ups) on this box's host cores. At N > 1 ``check`` compares
every rank's rows with the single-GPU conv of the global graph (on by default). Both gates also
hold the FIRST timed step — the one straight after the pre-timing barrier, its outputs kept — to
the same rule (``parity.first_step`` / ``check.first_step``); either failing fails the run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRIC = "hypergraph-conv fwd+bwd M-edges/sec at emb_dim=64; % HBM roofline"
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)

# users, items, edges per GPU (SURVEY.md §8 config sizes; dataset shapes are public statistics
# with the reference's 75 % train split, not shipped data)
WORKLOADS = {
    "synthetic": (10_000_000, 1_000_000, 100_000_000, None),
    "zipf": (10_000_000, 1_000_000, 100_000_000, 1.0),
    "ml1m": (6_040, 3_706, 750_000, None),
    "yelp": (31_668, 38_048, 1_170_000, None),
    "amazon": (52_643, 91_599, 2_240_000, None),
}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="synthetic", choices=sorted(WORKLOADS))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--users", type=int, default=None)
    ap.add_argument("--items", type=int, default=None)
    ap.add_argument("--edges", type=int, default=None)
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="strong: one global graph sharded by user rows (default); weak: one "
                         "full-size graph per rank")
    ap.add_argument("--chunks", type=int, default=4,
                    help="item-row chunks per exchanged column slice (N > 1): each chunk's "
                         "all-reduce is queued behind the hop-1 kernel that produced it")
    ap.add_argument("--slice-width", type=int, default=None,
                    help="embedding columns per pipelined all-reduce block (N > 1; default 32 "
                         "for d <= 128, else 64)")
    ap.add_argument("--transport", default="auto", choices=["auto", "rccl", "p2p"],
                    help="N > 1: the item-message all-reduce over RCCL (torch.distributed "
                         "'nccl') or the direct xGMI peer exchange (hgd_p2p: two-shot mesh "
                         "reduce over IPC-mapped buffers, sharded.P2PExchange); auto (default) "
                         "times both after the warm-up and runs the timed steps on the faster "
                         "(RCCL if the peer exchange fails or disagrees with it)")
    ap.add_argument("--check", action=argparse.BooleanOptionalAction, default=None,
                    help="after timing, compare the sharded Y / dX with the single-GPU conv of "
                         "the global graph (strong scaling) at the 1e-5 relative bound; on by "
                         "default when N > 1 (--no-check to skip)")
    ap.add_argument("--cpu-sample-frac", type=float, default=0.1,
                    help="share of the users (a prefix of the row-sorted graph) the CPU "
                         "baseline's timed runs cover; the parity gate always runs the full graph")
    ap.add_argument("--full", action="store_true",
                    help="N = 1: also everything that takes runs of its own beside the timed "
                         "steps: the rocprofv3 PMC passes, the stream-copy peak, the CPU "
                         "reference with its parity gate and the cpu_baseline (off by default: "
                         "a plain run sets up, warms up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's Y and dX (float32; "
                         "above the size budget a fixed seeded sample of rows) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full, skip the CPU reference: no cpu_baseline and no parity gate")
    ap.add_argument("--pmc", default="auto", choices=["auto", "on", "off"],
                    help="measure HBM traffic with rocprofv3 PMC passes in a child process "
                         "(auto: with --full at N = 1 on the synthetic and zipf workloads)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--graph", default="off", choices=["on", "off"],
                    help="replay the fwd+bwd step as one captured hipGraph (measured: no gain "
                         "once the per-hop events are out of the timed loop)")
    return ap.parse_args(argv)


def make_graph(U, I, E, seed, zipf, device):
    """Synthetic incidence on the device: uniform users, uniform (or Zipf) items, deduplicated,
    row-major sorted (torch generator seeded per rank; the bench's data, not the product)."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    u = torch.randint(0, U, (E,), device=device, generator=g, dtype=torch.int64)
    if zipf is None:
        i = torch.randint(0, I, (E,), device=device, generator=g, dtype=torch.int64)
    else:
        ranks = torch.arange(1, I + 1, device=device, dtype=torch.float64)
        p = ranks.pow(-float(zipf))
        i = torch.multinomial((p / p.sum()).float(), E, replacement=True, generator=g)
    key = torch.unique(u * I + i)
    del u, i
    return torch.stack([key // I, key % I])


def cpu_reference(idx, X, dY, U, I):
    """The reference's own library calls (oracle/ref_cpu.py: torch.sparse.mm fwd + autograd bwd,
    HCCF.py:199 on the data/graph.py:28-42 normalisation) on the FULL headline graph and the GPU
    run's X / dY, copied to the host: (Y, dX, seconds). The outputs are the parity gate's
    reference (BASELINE.md §3 "a speed-up is reported only if parity holds on the same run")."""
    import torch

    from oracle import ref_cpu
    H = torch.sparse_coo_tensor(idx, torch.ones(int(idx.shape[1]), dtype=torch.float32), (U, I))
    t0 = time.perf_counter()
    Y, dX = ref_cpu.hgconv2_fwd_bwd(H, X, dY)
    return Y, dX, time.perf_counter() - t0


def row_parity(got, ref, block=1 << 20):
    """The encoder-level rule of tests/_ref64.check_rows at any size: per row, max |got − ref|
    over the row's largest |ref| (in float64, in blocks of rows); an all-zero reference row
    must come out exactly zero. Returns (worst ratio, worst row, rows over 1e-5, zero-row
    violations)."""
    import torch
    worst, where, over, zero_bad = 0.0, -1, 0, 0
    for r0 in range(0, ref.shape[0], block):
        g = got[r0:r0 + block].double()
        r = ref[r0:r0 + block].double()
        err = (g - r).abs().amax(1)
        scale = r.abs().amax(1)
        zero = scale == 0
        zero_bad += int((err[zero] != 0).sum())
        ratio = torch.where(zero, torch.zeros_like(err), err / torch.where(zero, 1.0, scale))
        over += int((ratio > 1e-5).sum())
        m = float(ratio.max()) if ratio.numel() else 0.0
        if m > worst:
            worst, where = m, r0 + int(ratio.argmax())
    return worst, where, over, zero_bad


def parity_gate(Y, dX, Y_ref, dX_ref, cpu_s, first=None):
    """The GPU step's (Y, dX) — one eager step after timing, the same code the timed steps ran —
    against the reference's torch.sparse.mm (Y, dX) on the same full-size inputs. ``first``: the
    FIRST timed step's (Y, dX) (the step straight after the pre-timing barrier), held to the same
    rule under ``first_step``; the gate fails if either fails."""
    out = {"ok": True, "bound": "per row: max|err| <= 1e-5 * max|ref| (tests/_ref64.check_rows)",
           "reference": "oracle/ref_cpu.py torch.sparse.mm fwd+bwd, full graph, same X/dY",
           "reference_s": round(cpu_s, 2)}

    def rule(dst, got_Y, got_dX):
        for name, got, ref in (("Y", got_Y, Y_ref), ("dX", got_dX, dX_ref)):
            worst, row, over, zero_bad = row_parity(got, ref)
            dst[f"max_row_ratio_{name}"] = worst
            dst[f"rows_over_{name}"] = over + zero_bad
            if over or zero_bad or got.shape != ref.shape:
                dst["ok"] = False
                dst[f"worst_row_{name}"] = row

    rule(out, Y, dX)
    if first is not None:
        fs = {"ok": True, "what": "the first timed step (straight after the pre-timing barrier)"}
        rule(fs, *first)
        out["first_step"] = fs
        out["ok"] = out["ok"] and fs["ok"]
    out["rows"] = int(Y_ref.shape[0])
    return out


def host_cpus():
    """The host the CPU baseline runs on: os.cpu_count() (the whole machine), this process's
    affinity set, the cgroup CPU quota (cpu.max / cfs_quota_us, None when unlimited) and
    OMP_NUM_THREADS. ``threads`` = the affinity count, capped by the quota — on
    the GPU box the affinity set spans the whole machine while the box's share is its quota."""
    cpu_count = os.cpu_count()
    try:
        affinity = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        affinity = cpu_count
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, p = fh.read().split()[:2]
            if q != "max":
                quota = -(-int(q) // int(p))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fh:
                q = int(fh.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                p = int(fh.read())
            if q > 0:
                quota = -(-q // p)
        except (OSError, ValueError):
            pass
    threads = max(1, min(affinity, quota) if quota else affinity)
    return {"os_cpu_count": cpu_count, "affinity": affinity, "cgroup_cpu_quota": quota,
            "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"), "threads": threads}


def cpu_baseline(idx, X, dY, U, I, d, label, full_s, frac=0.1, host=None):
    """The CPU baseline's timing: the reference's calls
    (oracle/ref_cpu.py) on a BOUNDED sample of the same workload — the users [0, U·frac) of the
    GPU run's graph (a prefix of its row-sorted COO, every item kept) with their X / dY rows —
    median of 5 runs after 2 warm-ups at the host's thread count (:func:`host_cpus`), then one
    run at one thread. The sample is NOT the headline graph (its X table is a tenth as large);
    the full-size run the parity gate made is reported beside it (``full_size``)."""
    import psutil
    import torch

    from oracle import ref_cpu
    host = host or host_cpus()
    prev_threads = torch.get_num_threads()
    torch.set_num_threads(host["threads"])
    nnz_full = int(idx.shape[1])
    Us = max(1, int(U * frac))
    n = int(torch.searchsorted(idx[0].contiguous(), torch.tensor([Us])).item())
    H = torch.sparse_coo_tensor(idx[:, :n], torch.ones(n, dtype=torch.float32), (Us, I))
    Xs, dYs = X[:Us], dY[:Us]
    for _ in range(2):
        ref_cpu.hgconv2_fwd_bwd(H, Xs, dYs)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        ref_cpu.hgconv2_fwd_bwd(H, Xs, dYs)
        times.append(time.perf_counter() - t0)
    t = statistics.median(times)
    ram = psutil.virtual_memory().total / 2**30
    out = {
        "value": round(n / t / 1e6, 3),
        "unit": "M-edges/s",
        "cores": torch.get_num_threads(),
        "kind": "port",
        "sample": (f"a {frac:g} prefix SAMPLE, not the headline graph (the full graph is "
                   f"full_size): users [0, {Us}) of {label}: {Us}x{I}, {n} edges, d={d}, the GPU "
                   f"run's X / dY rows; torch.sparse.mm fwd+bwd (oracle/ref_cpu.py), median of 5 "
                   f"after 2 warm-ups, {t:.2f} s/run; host RAM {ram:.0f} GiB"),
        "host": host,
        "threads_note": ("threads = the affinity count capped by the cgroup CPU quota. 1 thread "
                         "~ N threads: aten::addmm (sparse COO x dense, torch.sparse.mm's CPU "
                         "kernel) walks the nonzeros in one serial loop and takes >90% of the "
                         "time (profiles/r06_cpu/cpu_reference_profile.txt)"),
    }
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t0 = time.perf_counter()
        ref_cpu.hgconv2_fwd_bwd(H, Xs, dYs)
        t1 = time.perf_counter() - t0
    finally:
        torch.set_num_threads(prev_threads)
    out["single_thread"] = {"value": round(n / t1 / 1e6, 3), "cores": 1,
                            "sample": f"the same sample, one run, {t1:.2f} s"}
    out["full_size"] = {"value": round(nnz_full / full_s / 1e6, 3), "cores": threads,
                        "sample": f"the whole headline graph, {nnz_full} edges, one run "
                                  f"(the parity gate's reference), {full_s:.2f} s"}
    return out


def pmc_traffic(args, U, I, E):
    """Runs this script under rocprofv3 twice (FETCH_SIZE, WRITE_SIZE) as a child process and
    returns HBM bytes per hop (one hgd_spmm call, the unit HopTimer prices; a call over rows
    wider than one column pass is several kernel dispatches, summed): (FETCH_SIZE·2 +
    WRITE_SIZE)·1024 (gfx950 FETCH_SIZE reads half the bytes of wide streaming reads:
    MI355X_MICROARCH.md §HBM). The child runs 1 warmup + 2 timed steps of 4 hops."""
    import csv
    import glob
    import shutil
    import tempfile
    rp = shutil.which("rocprofv3")
    if not rp:
        return None, "rocprofv3 not found"
    out = {}
    tmp = tempfile.mkdtemp(prefix="hgd_pmc_", dir=os.environ.get("TMPDIR", "/tmp"))
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = os.path.join(tmp, ctr)
        cmd = [rp, "--pmc", ctr, "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--pmc-child", "--steps", "2",
               "--warmup", "1", "--workload", args.workload, "--dim", str(args.dim),
               "--users", str(U), "--items", str(I), "--edges", str(E)]
        try:
            subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
        except Exception as exc:  # noqa: BLE001 — report, never fail the bench
            return None, f"rocprofv3 {ctr} pass failed: {exc}"
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            return None, f"no counter csv for {ctr}"
        vals = []
        with open(files[0]) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                if "hgd::spmm_" in name and row.get("Counter_Name") == ctr:
                    vals.append(float(row["Counter_Value"]))
        if not vals:
            return None, f"no spmm_kernel rows for {ctr}"
        out[ctr] = sum(vals) / (4 * (2 + 1))  # per hop: 4 hops x (2 steps + 1 warmup)
    shutil.rmtree(tmp, ignore_errors=True)
    traffic = (out["FETCH_SIZE"] * 2.0 + out["WRITE_SIZE"]) * 1024.0
    return traffic, f"FETCH_SIZE={out['FETCH_SIZE']:.0f}KB WRITE_SIZE={out['WRITE_SIZE']:.0f}KB per hop"


def copy_peak_gbps(device, n_bytes=1 << 30, reps=10):
    """Streaming ceiling of this box: a 1 GiB device-to-device copy (one read + one write
    stream), timed as torch's copy_ and as a float4-per-thread copy kernel (hgd_epilogue_apply
    with no activation); median of `reps` launches each, returns (best GB/s, {name: GB/s})."""
    import torch

    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    n = n_bytes // 4
    a = torch.ones(n, device=device)
    b = torch.empty_like(a)
    lib = nat.load()

    def hgd_copy():
        nat.check(lib.hgd_epilogue_apply(a.data_ptr(), n, nat.EPI_NONE, 0.0, b.data_ptr(),
                                         torch.cuda.current_stream(device).cuda_stream),
                  "hgd_epilogue_apply")

    rates = {}
    for name, fn in (("torch_copy_", lambda: b.copy_(a)), ("float4_copy_kernel", hgd_copy)):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        rates[name] = round(2.0 * n_bytes / (statistics.median(ts) * 1e-3) / 1e9, 1)
    del a, b
    return max(rates.values()), rates


DUMP_BUDGET_BYTES = 48 * 10**6  # --dump-outputs: all files of all ranks together
DUMP_SEED = 0


def dump_outputs(path, outputs, rank=0, world=1):
    """--dump-outputs: every [n, d] tensor of ``outputs`` (name → tensor, the last timed step's
    results) as ``path/<name>.npy`` in float32 (``<name>_rank<r>.npy`` at N > 1). A tensor whose
    share of DUMP_BUDGET_BYTES holds fewer than n rows is written as a sample of its rows: k of
    n drawn without replacement by numpy's default_rng(DUMP_SEED), ascending, so the same rows
    in every run and the same rows for tensors of the same shape. Returns the record for the
    result line."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    share = DUMP_BUDGET_BYTES // (max(1, world) * max(1, len(outputs)))
    suffix = "" if world == 1 else f"_rank{rank}"
    picked = {}
    files = {}
    for name, t in outputs.items():
        t = t.detach()
        n = int(t.shape[0])
        k = min(n, share // max(1, 4 * (t.numel() // max(1, n))))
        if k < n:
            if (n, k) not in picked:
                rows = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=k, replace=False))
                picked[(n, k)] = torch.from_numpy(rows).to(t.device)
            t = t.index_select(0, picked[(n, k)])
        arr = t.to(torch.float32).cpu().numpy()
        np.save(os.path.join(path, f"{name}{suffix}.npy"), arr)
        files[f"{name}{suffix}.npy"] = {"shape": list(arr.shape), "rows_of": n,
                                        "sampled": k < n}
    return {"dir": path, "what": "the last timed step's outputs", "dtype": "float32",
            "sample_seed": DUMP_SEED, "files": files}


def choose_transport(sh, eager_step, device, phase, n=3):
    """--transport auto: after the warm-up, n steps over RCCL and n over the peer exchange (its
    first step compared with RCCL's result), max over ranks; the timed steps then run on the
    faster. Any failure of the peer exchange on any rank — setup, a bounded wait, a timed-out
    exchange, a result off by more than 1e-5 of max |Y| — keeps RCCL on every rank."""
    import torch
    import torch.distributed as dist

    def timed():
        """n steps between a barrier pair, max over ranks: (ms per step, error or None, the last
        step's (Y, dX)). A failure on this rank alone (a poll that sees the error flag, a
        timed-out wait) is recorded, never raised: every rank still reaches the same barrier and
        all-reduce, so the collectives stay paired and agree() below decides on all ranks at
        once."""
        err = None
        last = None
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        try:
            for _ in range(n):
                last = eager_step()
            if sh.transport == "p2p":
                sh._p2p.wait()
                sh._p2p.check()
        except Exception as e:  # noqa: BLE001 — reported through agree()
            err = repr(e)[:400]
        try:
            torch.cuda.synchronize()  # a stalled exchange ends at its device wait bound
        except Exception as e:  # noqa: BLE001
            err = err or repr(e)[:400]
        dist.barrier()
        t = torch.tensor([(time.perf_counter() - t0) / n * 1e3], dtype=torch.float64,
                         device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()), err, last

    out = {"steps_each": n}

    def agree(err, key="p2p_error"):  # every rank learns whether any rank failed
        flag = torch.tensor([0 if err is None else 1], dtype=torch.int32, device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if err is not None:
            out[key] = err
        return int(flag.item()) == 0

    def rel_diff(a, b):
        return max(float((a[0].detach() - b[0]).abs().max() / b[0].abs().max().clamp_min(1e-30)),
                   float((a[1] - b[1]).abs().max() / b[1].abs().max().clamp_min(1e-30)))

    sh.transport = "rccl"
    first = eager_step()
    ms, rccl_err, last = timed()
    if not agree(rccl_err, "rccl_error"):  # the all-reduce path itself failed: no fallback
        raise RuntimeError(f"RCCL steps failed on some rank: {out.get('rccl_error')}")
    out["rccl_ms_per_step"] = round(ms, 4)
    # The reference for the peer exchange is the LAST all-reduce step, not the first: in the
    # one-device gloo rehearsal the first gloo step after the warm-up's barrier came out wrong
    # in about a third of the cases while the back-to-back steps after it agreed bitwise
    # (scripts/diag/diag_p2p_first.py, profiles/r05_scale/p2p_first/). Both are reported.
    Y_r, dX_r = last[0].detach(), last[1].detach()
    out["rccl_first_vs_last_rel_diff"] = rel_diff(first, (Y_r, dX_r))
    # the probe's first step came straight after the warm-up's barrier: if it differs from the
    # back-to-back steps after it, the run fails (line_status), whichever transport is chosen
    out["rccl_first_step_ok"] = out["rccl_first_vs_last_rel_diff"] <= 1e-5
    del first, last

    err = None
    try:  # one step, checked against RCCL's, before any collective timing
        sh.transport = "p2p"
        Y_p, dX_p = eager_step()
        sh._p2p.wait()
        sh._p2p.check()
        rel = rel_diff((Y_p, dX_p), (Y_r, dX_r))
        out["p2p_vs_rccl_max_rel_diff"] = rel
        if not rel <= 1e-5:
            raise RuntimeError(f"peer exchange differs from RCCL by {rel:.3e} of max |Y|")
    except Exception as e:  # noqa: BLE001 — any failure keeps RCCL, reported in the line
        err = repr(e)[:400]
    ok = agree(err)
    if ok:
        ms, err, _ = timed()
        ok = agree(err)
        if ok:
            out["p2p_ms_per_step"] = round(ms, 4)
    use_p2p = ok and out.get("p2p_ms_per_step", float("inf")) < out["rccl_ms_per_step"]
    sh.transport = "p2p" if use_p2p else "rccl"
    out["chosen"] = sh.transport
    if not ok:
        out["p2p_failed_on_some_rank"] = True
    return out


def launch_ranks(args) -> int:
    """Starts ``--gpus`` ranks of this script under torch.distributed.run as a CHILD process (no
    exec: this process has not touched the GPU and never will) and returns its exit status."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1", f"--master-port={port}",
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


ROW_BLOCK = 1 << 20


def table_rows(u0, u1, d, seed, device, bound=None):
    """Rows [u0, u1) of a synthetic [U, d] table: uniform(-bound, bound) (xavier_uniform_ on the
    global table, HCCF.py:164-169) or N(0, 1) when ``bound`` is None, generated in blocks of
    2^20 rows with one generator per block (seed, block), so a rank draws only its own rows and
    every rank sees the same global table."""
    import torch
    out = torch.empty(max(0, u1 - u0), d, device=device)
    b = u0 // ROW_BLOCK
    while b * ROW_BLOCK < u1:
        r0, r1 = b * ROW_BLOCK, (b + 1) * ROW_BLOCK
        g = torch.Generator(device=device).manual_seed(seed * 1_000_003 + b)
        blk = torch.empty(ROW_BLOCK, d, device=device)
        if bound is None:
            blk.normal_(generator=g)
        else:
            blk.uniform_(-bound, bound, generator=g)
        a, z = max(r0, u0), min(r1, u1)
        out[a - u0:z - u0] = blk[a - r0:z - r0]
        del blk
        b += 1
    return out


def compare_elementwise(got, ref, mag):
    """|got − ref| <= 1e-5 · mag per element (mag = the conv of |X|, so a near-cancelling element
    is held to its terms' scale): {max_abs_err, max_rel_err, ok}."""
    err = (got - ref).abs()
    return {"max_abs_err": float(err.max()) if err.numel() else 0.0,
            "max_rel_err": float((err / (mag + 1e-30)).max()) if err.numel() else 0.0,
            "ok": bool((err <= 1e-5 * mag + 1e-30).all())}


def check_against_single_gpu(idx, U, I, X_global, dY_global, Y, dX, u0, u1, first=None):
    """Strong scaling: this rank's sharded Y / dX rows against the single-GPU hgconv2 of the
    global graph (functional.hgconv2, no exchange) at |err| <= 1e-5 · (the same conv of |X|).
    ``(Y, dX)`` is one step after timing; ``first`` the FIRST timed step (straight after the
    pre-timing barrier), checked against the same reference under ``first_step``."""
    import torch

    from hypergraph_diffusion_for_recommendation_amd import Incidence, hgconv2
    inc = Incidence.from_coo(idx, None, (U, I), validate=False, rows_sorted=True)
    Xg = X_global.detach().clone().requires_grad_(True)
    Yg = hgconv2(inc, Xg)
    (dXg,) = torch.autograd.grad(Yg, Xg, dY_global)
    with torch.no_grad():
        mag = hgconv2(inc, X_global.abs())
        dmag = hgconv2(inc, dY_global.abs())  # the conv is self-adjoint: dX = conv(dY)
        return check_rows(Y, dX, Yg[u0:u1], dXg[u0:u1], mag[u0:u1], dmag[u0:u1], first)


def check_rows(Y, dX, Y_ref, dX_ref, mag_Y, mag_dX, first=None):
    """This rank's check record: the checked step's Y / dX and, when kept, the first timed
    step's (``first_step``) against the same reference rows (:func:`compare_elementwise`)."""
    out = {"Y": compare_elementwise(Y, Y_ref, mag_Y),
           "dX": compare_elementwise(dX, dX_ref, mag_dX)}
    if first is not None:
        out["first_step"] = {"Y": compare_elementwise(first[0], Y_ref, mag_Y),
                             "dX": compare_elementwise(first[1], dX_ref, mag_dX)}
    return out


def line_status(check, parity, probe=None) -> int:
    """Exit status of the run: 1 if the N > 1 check (either step), the N = 1 parity gate (either
    step) or the transport probe's first all-reduce step after the warm-up barrier failed, else
    0."""
    bad = (check is not None and not check["ok"]) or (parity is not None and not parity["ok"])
    bad = bad or (probe is not None and probe.get("rccl_first_step_ok") is False)
    return 1 if bad else 0


def corrupt_first_step(first, rank):
    """Rehearsal hook: HGD_BENCH_CORRUPT_FIRST_STEP=<rank> adds max|Y| + 1 to element 0 of that
    rank's kept first-step Y (after the timed region), so the first-step check must fail the
    line on hardware where the exchange is right."""
    if first is None or os.environ.get("HGD_BENCH_CORRUPT_FIRST_STEP") != str(rank):
        return first
    Y, dX = first
    if Y.numel():
        Y.view(-1)[0] += float(Y.abs().max()) + 1.0
    return Y, dX


def check_enabled(args, world) -> bool:
    """--check / --no-check; unset, an N > 1 record proves cross-device correctness by default."""
    return world > 1 if args.check is None else bool(args.check)


def gather_checks(check, world, shared_device):
    """Every rank's check_against_single_gpu result → the line's ``check`` (on every rank)."""
    import torch.distributed as dist
    checks = [None] * world
    dist.all_gather_object(checks, check)
    out = {"ok": all(c["Y"]["ok"] and c["dX"]["ok"] for c in checks),
           "max_rel_err_Y": max(c["Y"]["max_rel_err"] for c in checks),
           "max_rel_err_dX": max(c["dX"]["max_rel_err"] for c in checks),
           "bound": "|err| <= 1e-5 * conv(|x|), per element",
           "what": "one step after the timed steps",
           "ranks_checked": world,
           "wall_s": max(c.get("wall_s", 0.0) for c in checks),
           "ranks_in_parallel": not shared_device}
    firsts = [c.get("first_step") for c in checks]
    if all(f is None for f in firsts):
        out["first_step"] = None
    else:
        fs = [f for f in firsts if f is not None]
        bad = [q for q, f in enumerate(firsts)
               if f is None or not (f["Y"]["ok"] and f["dX"]["ok"])]
        out["first_step"] = {"ok": not bad, "failed_ranks": bad,
                             "max_rel_err_Y": max(f["Y"]["max_rel_err"] for f in fs),
                             "max_rel_err_dX": max(f["dX"]["max_rel_err"] for f in fs),
                             "what": "the first timed step, straight after the pre-timing "
                                     "barrier, on every rank"}
        out["ok"] = out["ok"] and not bad
    return out


def main():
    args = parse()
    U0, I0, E0, zipf = WORKLOADS[args.workload]
    U = args.users or U0
    I = args.items or I0
    E = args.edges or E0
    d = args.dim

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}; refusing to report a "
              f"mislabelled run", file=sys.stderr)
        sys.exit(2)
    strong = args.scaling == "strong"
    args.check = check_enabled(args, world)
    t_launch = time.perf_counter()

    stall_s = float(os.environ.get("HGD_STALL_DUMP_S", "600"))
    watchdog = [False]

    def phase(msg):  # multi-rank progress on stderr (rehearsals of N ranks on one device)
        if world > 1:
            print(f"[bench rank {rank}] {time.perf_counter() - t_launch:7.1f} s {msg}",
                  file=sys.stderr, flush=True)
            if watchdog[0]:  # progress: the stall dump fires only HGD_STALL_DUMP_S after it
                import faulthandler
                faulthandler.cancel_dump_traceback_later()
                faulthandler.dump_traceback_later(stall_s, exit=False)

    pmc = None
    pmc_note = None
    want_pmc = (args.pmc == "on" or (args.pmc == "auto" and args.full and world == 1
                                     and args.workload in ("synthetic", "zipf")))
    if want_pmc and not args.pmc_child:
        # child profiler processes run BEFORE this process touches the GPU
        pmc, pmc_note = pmc_traffic(args, U, I, E)

    import torch
    import torch.distributed as dist

    from hypergraph_diffusion_for_recommendation_amd import Incidence, profiling
    from hypergraph_diffusion_for_recommendation_amd.sharded import (ExchangeTimer,
                                                                       ShardedIncidence,
                                                                       init_process_group,
                                                                       sharded_two_hop)

    # one rank per GPU; the modulo only matters for rehearsing N ranks on fewer GPUs (gloo)
    dev_index = local_rank % max(1, torch.cuda.device_count())
    device = torch.device(f"cuda:{dev_index}")
    torch.cuda.set_device(device)
    dist_backend = None
    phase("torch imported")
    if world > 1:
        dist_backend = os.environ.get("HGD_DIST_BACKEND", "nccl")  # nccl == RCCL
        init_process_group(device, dist_backend)
        phase("process group up")

    if world > 1:
        # a rank that stops making progress prints every thread's Python stack (the line it is
        # blocked in) instead of dying silently at the launcher's limit; re-armed by every
        # phase() line, so a long run that keeps reporting progress never dumps
        import faulthandler
        faulthandler.dump_traceback_later(stall_s, exit=False)
        watchdog[0] = True
    shard_kw = dict(n_chunks=args.chunks, P="sym", Q="mean", R="sym",
                    slice_width=args.slice_width,
                    transport="rccl" if args.transport == "auto" else args.transport,
                    trace=phase if world > 1 else None)
    bound = (6.0 / (U + d)) ** 0.5  # xavier_uniform_ on the global [U, d] (HCCF.py:164-169)
    keep_global = args.check and strong and world > 1
    # N ranks rehearsed on fewer devices: the graph builds (a 100 M-key sort each) run one rank
    # at a time — eight at once on one device took 7-10 minutes instead of 8 × 15 s. (Only the
    # build: the shard set-up below all-reduces the item degrees, so it runs on every rank at once.)
    shared_device = world > 1 and torch.cuda.device_count() < world
    for turn in range(world if shared_device else 1):
        if not shared_device or turn == rank:
            idx = make_graph(U, I, E, seed=0 if strong else rank, zipf=zipf, device=device)
            torch.cuda.synchronize()
            phase(f"graph built ({int(idx.shape[1])} edges)")
        if shared_device:
            dist.barrier()
    nnz_graph = int(idx.shape[1])
    u0, u1 = 0, U
    if strong and world > 1:
        sh, u0, u1 = ShardedIncidence.from_global(idx, U, I, device=device, **shard_kw)
        inc = sh.inc
    else:
        inc = Incidence.from_coo(idx, None, (U, I), device=device, validate=False,
                                 rows_sorted=True)
        sh = ShardedIncidence(inc, **shard_kw)
    want_cpu = (args.full and not args.no_cpu_baseline and world == 1
                and not args.pmc_child)
    idx_host = idx.cpu() if want_cpu else None  # the CPU baseline runs on the same graph
    if not keep_global:
        del idx
    nnz = inc.nnz
    phase(f"shard ready ({nnz} edges, users [{u0}, {u1}))")
    seed_x = 1000 + (0 if strong else rank)
    X = table_rows(u0, u1, d, seed_x, device, bound)
    dY = table_rows(u0, u1, d, seed_x + 1, device)
    X.requires_grad_(True)
    # warm the scale / edge-value caches outside the timed region
    inc.scale("row", "sym"), inc.edge_values("csc", "sym")

    def eager_step():
        Y = sharded_two_hop(sh, X)
        (dX,) = torch.autograd.grad(Y, X, dY)
        return Y, dX

    step = eager_step
    use_graph = args.graph == "on"
    if use_graph:
        if world > 1:
            raise SystemExit("bench.py: --graph on is single-GPU only (RCCL calls are not "
                             "captured here)")
        # whole-step capture: fwd + autograd bwd (4 hgd_spmm launches and their allocations) as
        # one hipGraph over the static X / dY — replay removes the host launch overhead that
        # dominates dataset-sized graphs, with no input copies (make_graphed_callables would
        # copy X and dY into placeholders every replay: 2 × 2.56 GB at the 100 M-edge shape)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(3):
                eager_step()
        torch.cuda.current_stream(device).wait_stream(side)
        import gc
        gc.collect()  # no eager autograd graph (its nodes bound to another stream) may survive
        graph = torch.cuda.CUDAGraph()
        # thread-local capture: the autograd engine runs the backward on its device thread, and
        # under this build's default ("global") mode the capture then ends in a crash
        # (scripts/diag/diag_graph_capture.py: torch ops alone crash the same way)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            static_out = eager_step()

        def step():
            graph.replay()
            return static_out

    # the first timed step's (Y, dX) are kept for the checks (an eager step's outputs; a graph
    # replay overwrites its static outputs)
    keep_first = (args.check or want_cpu) and not use_graph and not args.pmc_child
    # --dump-outputs: the last timed step's (Y, dX), held (no copy) until they are written
    want_dump = args.dump_outputs is not None and not args.pmc_child
    last_out = [None]
    prev = None
    for k in range(args.warmup):
        # each warm-up step's outputs live until the next one's exist, so the allocator caches
        # the blocks of two steps' outputs: holding the first timed step's costs no allocation
        # inside the timed region
        out_k = step()
        prev = out_k if keep_first else None
        del out_k
        phase(f"warm-up step {k} issued")
        if sh.transport == "p2p" and world > 1:
            sh._p2p.wait()  # bounded: a stalled exchange raises here instead of hanging
            sh._p2p.check()
    del prev
    torch.cuda.synchronize()
    phase("warm")
    if world > 1:
        dist.barrier()
    probe = None
    if world > 1 and args.transport == "auto":
        probe = choose_transport(sh, eager_step, device, phase)
        phase(f"transport: {probe}")
    def timed_and_checked():
        """The timed steps (barrier + sync both sides), then — with --check — one more step
        compared with the single-GPU conv of the global graph, and the FIRST timed step (the
        one straight after the barrier, kept) compared with it too. Returns (elapsed s, hop
        summary, hop ms / step, exposed exchange ms / step, this rank's check or None, error or
        None, the first step's (Y, dX) or None); a failure of the peer exchange on this rank is
        returned, never raised, so every rank reaches the same collectives."""
        # roofline: HIP events around every hop launch on its stream, recorded inside the timed
        # region (two event records per hop, a few µs on a ~16 ms step); a captured graph cannot
        # record them, so with --graph on the same steps are re-run eagerly afterwards for them
        timer = profiling.HopTimer()
        xtimer = ExchangeTimer()
        failure = None
        first = None
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        try:
            last_out[0] = None
            if use_graph:
                for _ in range(args.steps):
                    out_k = step()
                if want_dump and args.steps > 0:
                    last_out[0] = (out_k[0].detach(), out_k[1])  # the replay's static outputs
            else:
                with timer, xtimer:
                    for k in range(args.steps):
                        out_k = step()
                        if k == 0 and keep_first:
                            first = (out_k[0].detach(), out_k[1])
                        if want_dump and k == args.steps - 1:
                            last_out[0] = (out_k[0].detach(), out_k[1])
                        del out_k
        except Exception as e:  # noqa: BLE001 — a bounded p2p wait; agreed on below
            if sh.transport != "p2p":
                raise
            failure = repr(e)[:400]
        try:
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            if sh.transport != "p2p":
                raise
            failure = failure or repr(e)[:400]
        if world > 1:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        if use_graph:
            with timer:
                for _ in range(args.steps):
                    eager_step()
            torch.cuda.synchronize()
        hop = timer.summary()
        if sh.transport == "p2p" and world > 1 and failure is None:
            try:
                sh._p2p.check()  # no exchange timed out
            except Exception as e:  # noqa: BLE001
                failure = repr(e)[:400]
        first = corrupt_first_step(first, rank)
        check = None
        if args.check and not args.pmc_child and failure is None:
            t_check = time.perf_counter()
            Y, dX = eager_step()
            Y = Y.detach()
            torch.cuda.synchronize()
            if keep_global:
                # every rank recomputes the global conv on its own device at once; ranks sharing
                # a device take turns (the single-GPU reference needs the whole [U, d] tables,
                # 10 GB each at d = 256, too much for N ranks on one device)
                for r in (range(world) if shared_device else [rank]):
                    if r == rank:
                        X_global = table_rows(0, U, d, seed_x, device, bound)
                        dY_global = table_rows(0, U, d, seed_x + 1, device)
                        check = check_against_single_gpu(idx, U, I, X_global, dY_global, Y, dX,
                                                         u0, u1, first=first)
                        del X_global, dY_global
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        phase(f"checked: {check}")
                    if shared_device:
                        dist.barrier()
                check["wall_s"] = round(time.perf_counter() - t_check, 2)
        return (elapsed, hop, hop["total_ms"] / args.steps, xtimer.total_ms() / args.steps,
                check, failure, first)

    elapsed, hop, hop_ms_step, exposed_ms_step, check, failure, first = timed_and_checked()
    fallback = None
    if world > 1 and sh.transport == "p2p":
        # the peer exchange chose by the probe must also pass the timed run's own check on
        # every rank; otherwise the timed steps and the check are redone over RCCL and the line
        # says why (a wrong exchange is never reported as a result)
        bad = failure is not None or (check is not None and not (check["Y"]["ok"]
                                                                 and check["dX"]["ok"]))
        # rehearsal hook: HGD_BENCH_FAIL_P2P_CHECK=1 treats this rank's p2p check as failed, so
        # the fallback below runs on hardware where the exchange is right
        bad = bad or os.environ.get("HGD_BENCH_FAIL_P2P_CHECK") == "1"
        flag = torch.tensor([1 if bad else 0], dtype=torch.int32, device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if int(flag.item()):
            fallback = {"from": "p2p", "to": "rccl",
                        "reason": failure or "p2p check failed on some rank"}
            phase(f"transport fallback: {fallback}")
            sh.transport = "rccl"
            for k in range(args.warmup):
                step()
            torch.cuda.synchronize()
            del first
            (elapsed, hop, hop_ms_step, exposed_ms_step, check, failure,
             first) = timed_and_checked()
            if failure is not None:
                raise RuntimeError(f"RCCL timed steps failed: {failure}")
    dumped = None
    if want_dump and last_out[0] is not None:
        dumped = dump_outputs(args.dump_outputs, {"Y": last_out[0][0], "dX": last_out[0][1]},
                              rank, world)
    last_out[0] = None
    if keep_global:
        del idx
    per_rank = [{"rank": rank, "users": [u0, u1], "nnz": nnz, "hop_ms_per_step":
                 round(hop_ms_step, 4), "exposed_exchange_ms_per_step":
                 round(exposed_ms_step, 4)}]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        gathered = [None] * world
        dist.all_gather_object(gathered, per_rank[0])
        per_rank = gathered
        if check is not None:
            check = gather_checks(check, world, shared_device)
    total_edges = float(nnz_graph if strong else sum(r["nnz"] for r in per_rank))
    if strong and world > 1:
        assert sum(r["nnz"] for r in per_rank) == nnz_graph, "shards do not tile the graph"

    if args.pmc_child:
        return
    if rank != 0:
        if world > 1:
            dist.barrier()
            sh.close()
            dist.destroy_process_group()
        return finish(0)

    value = total_edges * args.steps / elapsed / 1e6
    achieved = hop["avg_bytes"] / (hop["avg_ms"] * 1e-3) / 1e9 if hop["avg_ms"] > 0 else 0.0
    roofline = {
        "bound": "hbm",
        "achieved": round(achieved, 1),
        "peak": HBM_PEAK_GBPS,
        "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBPS, 4),
        "traffic": None if pmc is None else round(pmc / 1.0),
        "kernel": "hgd::spmm_kernel (hgd_spmm hop)",
        "algorithmic_bytes_per_launch": round(hop["avg_bytes"]),
        "algorithmic_model": profiling.MODEL_NOTE,
        "implementation_bytes_per_launch": round(hop["avg_impl_bytes"]),
        "avg_launch_ms": round(hop["avg_ms"], 4),
        "launches_timed": hop["launches"],
    }
    # a "launch" above is one hop (one spmm_csr call); rocprofv3 lists spmm_kernel per dispatch:
    # hgd_spmm runs a row wider than 128 as 64-column passes, and the hop into items runs as
    # hgd_spmm_blocked (128-column passes) in `blocks` dispatches per pass when its gathered
    # user table exceeds the Infinity Cache (incidence.spmm_blocks)
    # (N = 1 only: the sharded hop at N > 1 runs column slices, blocked by their own width,
    # and never blocks into the peer exchange's slots)
    from hypergraph_diffusion_for_recommendation_amd.incidence import spmm_blocks
    blocks = spmm_blocks(sh.inc.csc, args.dim) if world == 1 else 0
    passes = 1 if args.dim <= 128 else -(-args.dim // 64)  # hgd_spmm's 64-column passes
    bpasses = -(-args.dim // 128)  # hgd_spmm_blocked's 128-column passes
    if world == 1:
        roofline["dispatches_per_hop"] = {"into_items": bpasses * blocks if blocks else passes,
                                          "into_users": passes}
    if blocks:
        roofline["kernel"] = ("hgd::spmm_kernel (hgd_spmm hop; into items: hgd_spmm_blocked, "
                              f"{blocks} source blocks)")
    # per-hop breakdown: launches cycle fwd-CSC (into items), fwd-CSR (into users), bwd-CSC, bwd-CSR
    names = ["fwd_items", "fwd_users", "bwd_items", "bwd_users"]
    if world == 1 and hop["launches"] % 4 == 0:
        per = {}
        for k, nm in enumerate(names):
            ms = hop["per_launch_ms"][k::4]
            by = hop["per_launch_bytes"][k::4]
            per[nm] = {"ms": round(statistics.mean(ms), 4),
                       "GBps": round(statistics.mean(by) / (statistics.mean(ms) * 1e-3) / 1e9, 1)}
        roofline["per_hop"] = per
        # the hop into items gathers the user table (U·d·4 bytes, far beyond any cache) at random:
        # its rate is the HBM-efficiency figure; the hop into users gathers the item table, which
        # is partly Infinity-Cache resident, so the mean over both is cache-assisted
        items = [per[nm]["GBps"] for nm in ("fwd_items", "bwd_items")]
        roofline["frac_uncached_hop"] = round(statistics.mean(items) / HBM_PEAK_GBPS, 4)
        roofline["frac_note"] = ("frac is the mean over all four hops; the hops into users read "
                                 "a partly cache-resident item table, frac_uncached_hop is the "
                                 "into-items hops alone (gathering the user table; when blocked, "
                                 "dispatches_per_hop.into_items > 1, each dispatch's user slice "
                                 "is partly cache-resident too)")
    if world == 1 and args.full:
        # also report a measured stream-copy peak on this box (read + write bytes)
        cp, cp_detail = copy_peak_gbps(device)
        roofline["measured_copy_GBps"] = round(cp, 1)
        roofline["measured_copy_detail"] = cp_detail
        roofline["frac_of_measured_copy"] = round(achieved / cp, 4) if cp > 0 else None
    if pmc_note:
        roofline["traffic_note"] = pmc_note
    if pmc is not None:
        roofline["traffic_over_algorithmic"] = round(pmc / hop["avg_bytes"], 3)
        roofline["frac_by_traffic"] = round(pmc / (hop["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                                            4)

    cpu = parity = None
    if want_cpu:
        # the parity gate: one more eager step of the timed code, then the reference's own
        # torch.sparse.mm fwd+bwd on the same full graph and tables, compared row by row
        Yg, dXg = eager_step()
        Yh, dXh = Yg.detach().cpu(), dXg.cpu()
        first_h = None if first is None else (first[0].cpu(), first[1].cpu())
        Xh, dYh = X.detach().cpu(), dY.cpu()
        del X, dY, Yg, dXg, first
        torch.cuda.empty_cache()
        host = host_cpus()
        threads0 = torch.get_num_threads()
        torch.set_num_threads(host["threads"])
        try:
            Y_ref, dX_ref, full_s = cpu_reference(idx_host, Xh, dYh, U, I)
        finally:
            torch.set_num_threads(threads0)
        parity = parity_gate(Yh, dXh, Y_ref, dX_ref, full_s, first=first_h)
        del Yh, dXh, Y_ref, dX_ref, first_h
        cpu = cpu_baseline(idx_host, Xh, dYh, U, I, d, f"{args.workload}-{U}x{I}x{E}-d{d}",
                           full_s, args.cpu_sample_frac, host=host)
        del idx_host, Xh, dYh

    if world == 1:
        parallelism = "single GPU"
    elif sh.transport == "p2p":
        parallelism = (f"user-row shards x{world} ({'one global graph' if strong else 'a graph per rank'}), "
                       f"direct xGMI peer all-reduce (hgd_p2p two-shot mesh reduce, "
                       f"{dist_backend} for setup) of item messages in {len(sh.slices(d))} "
                       f"column slices, pipelined with the hops on a high-priority side stream")
    else:
        parallelism = (f"user-row shards x{world} ({'one global graph' if strong else 'a graph per rank'}), "
                       f"{'RCCL' if dist_backend == 'nccl' else dist_backend} all-reduce of item "
                       f"messages in {len(sh.slices(d))} column slices x {len(sh.bounds)} "
                       f"item chunks, pipelined with the hops")
    out = {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "M-edges/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f32",
        "data": (f"synthetic: uniform{'' if zipf is None else '/Zipf items'} user x item "
                 f"incidence (torch generator seed={'0, one global graph' if strong else 'rank'}"
                 f", dedup), xavier_uniform X, N(0,1) dY"),
        "config": {
            "workload": f"{args.workload}-{U}x{I}x{E}-d{d}",
            "users": U, "items": I, "edges_requested": E,
            "edges": int(total_edges), "emb_dim": d,
            "op": "hgconv2 fwd+bwd: D_v^-1/2 H D_e^-1 H^T D_v^-1/2 X, 4 hgd_spmm hops",
            "parallelism": parallelism,
            "hip_graph": use_graph,
        },
        "roofline": roofline,
        "cpu_baseline": cpu,
    }
    if world > 1:
        out["ranks"] = per_rank
        out["exchange_bytes_per_step"] = 2 * sh.exchange_bytes(d)
        out["transport"] = sh.transport
        if probe is not None:
            out["transport_probe"] = probe
        if fallback is not None:
            out["transport_fallback"] = fallback
        # the time the compute stream waited for the all-reduces (HIP events around every hop-2
        # wait), max over ranks: 0 = the exchange was hidden behind the hops
        out["exposed_exchange_ms_per_step"] = max(r["exposed_exchange_ms_per_step"]
                                                  for r in per_rank)
    if check is not None:
        out["check"] = check
    if world == 1:
        out["parity"] = parity
    out["full"] = bool(args.full)
    if dumped is not None:
        out["dump_outputs"] = dumped
    print(json.dumps(out), flush=True)
    if parity is not None and not parity["ok"]:
        print(f"bench.py: PARITY FAILED against the reference's torch.sparse.mm on the same "
              f"inputs: {parity}", file=sys.stderr, flush=True)
    if world > 1:
        dist.barrier()
        sh.close()
        dist.destroy_process_group()
    if check is not None and not check["ok"]:
        print(f"bench.py: CHECK FAILED against the single-GPU conv of the global graph: {check}",
              file=sys.stderr, flush=True)
    if probe is not None and probe.get("rccl_first_step_ok") is False:
        print(f"bench.py: the transport probe's first all-reduce step after the barrier differs "
              f"from the steps after it by {probe['rccl_first_vs_last_rel_diff']:.3e} of max |Y|",
              file=sys.stderr, flush=True)
    finish(line_status(check, parity, probe))


def finish(rc: int):
    """Exit status of a rank. A peer-exchange set-up call that never returned (the auto probe
    then chose RCCL) is still blocked on a daemon thread, and the HIP runtime's teardown at
    interpreter exit may wait for it: such a rank ends with os._exit once its output is out."""
    import faulthandler
    faulthandler.cancel_dump_traceback_later()
    from hypergraph_diffusion_for_recommendation_amd.sharded import p2p_setup_stuck
    if p2p_setup_stuck():
        print(f"bench.py: {p2p_setup_stuck()} peer-exchange set-up call(s) never returned; "
              f"exiting without runtime teardown", file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(rc)
    if rc:
        sys.exit(rc)


if __name__ == "__main__":
    main()
