#!/usr/bin/env python3
"""Unified CF + KG sampler, one epoch (host only): sampler.next_batch_unified (libhgd) against
the restated reference generator (tests/_unified_ref.py, util/sampler.py:7-90) on the same
inputs, in interleaved rounds; median and range per side.

Shapes: lastfm-like (KHGRec.conf: batch 2,048, KG batch 8,192) and Yelp2018-like. The reference
rebuilds its triple table in a Python loop per batch, so where a whole reference epoch would take
hours (--ref-batches > 0) it is timed over its epoch set-up plus that many batches and the epoch
is extrapolated from the per-batch time; the record says which. The native side always runs whole
epochs; its first epoch (which builds the cached host tables) is reported apart, and its epoch
set-up (time to the first batch: the two shuffles, CPython's two set orders, the NumPy tables)
apart from the per-batch draws. Prints one JSON line per shape."""
import argparse
import json
import os
import random
import statistics
import sys
import time
from collections import defaultdict
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _unified_ref as R  # noqa: E402
from hypergraph_diffusion_for_recommendation_amd.sampler import next_batch_unified  # noqa: E402

SHAPES = {
    # users, items, records, raw KG triples, further entities, relations, batch, KG batch, ref batches
    "lastfm_like": (1_891, 14_777, 70_000, 100_000, 20_000, 9, 2_048, 8_192, 0),
    "yelp2018_like": (31_668, 38_048, 1_170_000, 1_850_000, 45_000, 42, 4_096, 8_192, 2),
}


def make(n_users, n_items, n_records, n_kg, n_extra, n_rel, seed=0):
    """Users and items share one id space with the entities, as the KG carriers' files do: users
    first, then items, then the further entities."""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, n_users, n_records)
    items = rng.zipf(1.2, n_records) % n_items + n_users
    td = [[int(u), int(i), 1.0] for u, i in zip(users, items)]
    user, item, tsu = {}, {}, defaultdict(dict)
    for u, i, r in td:
        user.setdefault(u, len(user))
        item.setdefault(i, len(item))
        tsu[u][i] = r
    data = SimpleNamespace(training_data=td, user=user, item=item, training_set_u=tsu)
    h = rng.integers(n_users, n_users + n_items, n_kg)
    t = rng.integers(n_users, n_users + n_items + n_extra, n_kg)
    r = rng.integers(0, n_rel, n_kg)
    return data, (h, r, t)


def seed(s):
    random.seed(s)
    np.random.seed(s)


def time_epoch(gen, max_batches=0):
    t0 = time.perf_counter()
    first = None
    n = 0
    for _ in gen:
        n += 1
        if first is None:
            first = time.perf_counter() - t0
        if max_batches and n == max_batches:
            break
    return time.perf_counter() - t0, first, n


def stats(xs):
    return {"median_s": round(statistics.median(xs), 4), "min_s": round(min(xs), 4),
            "max_s": round(max(xs), 4)}


def run(name, rounds):
    n_users, n_items, n_records, n_kg, n_extra, n_rel, batch, batch_kg, ref_batches = SHAPES[name]
    data, (h, r, t) = make(n_users, n_items, n_records, n_kg, n_extra, n_rel)
    t0 = time.perf_counter()
    know = R.knowledge(data.training_data, h, r, t)
    t_know = time.perf_counter() - t0
    n_batches = -(-n_records // batch)
    out = {"shape": name, "users": n_users, "items": n_items, "records": n_records,
           "kg_triples_raw": n_kg, "n_kg_train": know.n_kg_train, "batch": batch,
           "batch_kg": batch_kg, "batches_per_epoch": n_batches, "rounds": rounds,
           "restated_knowledge_tables_s": round(t_know, 2)}
    seed(0)
    out["native_first_epoch_s"] = round(
        time_epoch(next_batch_unified(data, know, batch, batch_kg))[0], 4)
    ref_t, ref_first, nat_t, nat_first = [], [], [], []
    for k in range(rounds):
        seed(k + 1)
        tot, first, n = time_epoch(R.next_batch_unified(data, know, batch, batch_kg), ref_batches)
        if ref_batches:  # set-up + (time per further batch) × the epoch's batches
            per = (tot - first) / max(n - 1, 1)
            tot = first + per * (n_batches - 1)
        ref_t.append(tot)
        ref_first.append(first)
        seed(k + 1)
        tot, first, n = time_epoch(next_batch_unified(data, know, batch, batch_kg))
        assert n == n_batches
        nat_t.append(tot)
        nat_first.append(first)
    out["reference_epoch"] = dict(stats(ref_t), extrapolated_from_batches=ref_batches or None)
    out["reference_to_first_batch"] = stats(ref_first)
    out["native_epoch"] = stats(nat_t)
    out["native_to_first_batch"] = stats(nat_first)
    out["native_per_batch_ms"] = round(
        1e3 * statistics.median((a - b) / max(n_batches - 1, 1) for a, b in zip(nat_t, nat_first)),
        3)
    out["speedup_median"] = round(out["reference_epoch"]["median_s"]
                                  / out["native_epoch"]["median_s"], 1)
    out["speedup_worst_case"] = round(min(ref_t) / max(nat_t), 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    for name in args.shapes:
        run(name, args.rounds)


if __name__ == "__main__":
    main()
