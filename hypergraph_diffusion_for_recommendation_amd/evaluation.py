"""Batched scoring + top-K recommendation lists.

Replaces the per-user loop of ``GraphRecommender.test()`` (base/graph_recommender.py:61-92 in the
reference): for each test user ``predict(u)`` = ``user_emb[u] @ item_emb.T`` copied to the host,
rated items set to -10e8, then numba ``find_k_largest`` (util/algorithm.py:143-173). Here users
are scored in batches with one library GEMM (rocBLAS via torch.mm), the rated items are masked
by ``hgd_mask_scores`` and the lists come from ``hgd_topk_rows``, which reproduces
find_k_largest's ordering exactly — including its duplicated entries for top items among the
first K candidates. Only the [n_users, K] result crosses to the host. ``fused=True`` ranks with
``hgd_rank_topk`` instead: one kernel from the two tables and the rated-items CSR to the lists,
with no score matrix (opt-in).
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as nat
from .incidence import CSR

MASK_VALUE = -10e8  # base/graph_recommender.py:80


def rated_csr(interaction_mat, device) -> CSR:
    """Rated items per user (the training interactions, ``data.user_rated``) as a device CSR
    from the reference's ``data.interaction_mat`` (scipy [n_users, n_items])."""
    m = interaction_mat.tocsr()
    rowptr = torch.from_numpy(m.indptr.astype(np.int64)).to(device)
    col = torch.from_numpy(m.indices.astype(np.int32)).to(device)
    return CSR(rowptr, col, m.shape[0], m.shape[1], split_threshold=0)


def topk_rows(scores: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """find_k_largest(k, row) for every row of a device fp32 score matrix."""
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.device.type != "cuda":
        raise TypeError("topk_rows: expects a 2-D float32 device tensor")
    if scores.stride(1) != 1:
        scores = scores.contiguous()
    n, m = scores.shape
    ids = torch.empty((n, k), dtype=torch.int32, device=scores.device)
    vals = torch.empty((n, k), dtype=torch.float32, device=scores.device)
    nat.check(nat.load().hgd_topk_rows(scores.data_ptr(), n, m, scores.stride(0), int(k),
                                       ids.data_ptr(), vals.data_ptr(),
                                       nat.stream_handle(scores.device)),
              "hgd_topk_rows")
    return ids, vals


def mask_scores(scores: torch.Tensor, rated: CSR, users: torch.Tensor,
                value: float = MASK_VALUE) -> torch.Tensor:
    """In place: scores[r, rated items of users[r]] = value."""
    row_map = users.to(device=scores.device, dtype=torch.int32).contiguous()
    nat.check(nat.load().hgd_mask_scores(
        scores.data_ptr(), scores.shape[0], scores.stride(0), rated.rowptr.data_ptr(),
        rated.col.data_ptr() if rated.nnz else None, row_map.data_ptr(), float(value),
        nat.stream_handle(scores.device)), "hgd_mask_scores")
    return scores


SCORE_BUFFER_BYTES = 4 << 30  # default user batch: as many score rows as fit in 4 GiB
RANK_MAX_K, RANK_MAX_D = 64, 256  # HGD_RANK_MAX_K / HGD_RANK_MAX_D (include/hgd.h)
FUSED_BATCH = 1 << 16  # default rows per hgd_rank_topk launch (bounds the workspace)


def _check_table(name: str, t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
        raise TypeError(f"rank_users(fused=True): {name} must be a 2-D float32 device tensor")


@torch.no_grad()
def rank_users_fused(user_emb: torch.Tensor, item_emb: torch.Tensor, users: torch.Tensor,
                     rated: Optional[CSR], k: int, batch: Optional[int] = None,
                     segments: Optional[int] = None,
                     value: float = MASK_VALUE) -> Tuple[torch.Tensor, torch.Tensor]:
    """hgd_rank_topk: the lists of :func:`rank_users` without a score matrix. The scores are the
    kernel's own fp32 products (f32 MFMA), so they can differ from the library GEMM's in the last
    bits; ``batch`` only bounds the rows per launch and ``segments`` (None = by shape) only the
    split of the catalogue over workgroups — the result depends on neither."""
    _check_table("user_emb", user_emb)
    _check_table("item_emb", item_emb)
    k = int(k)
    n_items, d = int(item_emb.shape[0]), int(item_emb.shape[1])
    if user_emb.shape[1] != d:
        raise ValueError(f"rank_users(fused=True): widths {user_emb.shape[1]} and {d} differ")
    if k > RANK_MAX_K:
        raise ValueError(f"rank_users(fused=True): k = {k} exceeds HGD_RANK_MAX_K = {RANK_MAX_K}")
    if d > RANK_MAX_D:
        raise ValueError(f"rank_users(fused=True): d = {d} exceeds HGD_RANK_MAX_D = {RANK_MAX_D}")
    if k < 1 or k > n_items:
        raise ValueError(f"rank_users(fused=True): k = {k} of {n_items} items")
    nseg = 0 if segments is None else int(segments)
    if nseg < 0:
        raise ValueError("rank_users(fused=True): segments must be >= 0")
    for name, t in (("user_emb", user_emb), ("item_emb", item_emb)):
        if t.device.type != "cuda":  # no CPU path
            raise TypeError(f"rank_users(fused=True): {name} must be a 2-D float32 device "
                            "tensor (it is on the host)")
    if user_emb.stride(1) != 1:
        user_emb = user_emb.contiguous()
    if item_emb.stride(1) != 1:
        item_emb = item_emb.contiguous()
    dev = user_emb.device
    users = users.to(device=dev, dtype=torch.int32).contiguous()
    n = users.numel()
    out_ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    out_sc = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return out_ids, out_sc
    rowptr = cols = None
    if rated is not None:
        rowptr, cols = rated.rowptr, rated.ascending_col()
    step = max(1, int(batch)) if batch is not None else FUSED_BATCH
    lib = nat.load()
    ws = torch.empty(max(1, lib.hgd_rank_topk_workspace_size(min(step, n), n_items, k, nseg)),
                     dtype=torch.uint8, device=dev)
    for b0 in range(0, n, step):
        rows = min(step, n - b0)
        nat.check(lib.hgd_rank_topk(
            user_emb.data_ptr(), user_emb.stride(0), item_emb.data_ptr(), item_emb.stride(0),
            n_items, d, users[b0:].data_ptr(), rows, nat.ptr(rowptr),
            cols.data_ptr() if cols is not None and cols.numel() else None, float(value), k, nseg,
            out_ids[b0:].data_ptr(), out_sc[b0:].data_ptr(), ws.data_ptr(), ws.numel(),
            nat.stream_handle(dev)), "hgd_rank_topk")
    return out_ids, out_sc


@torch.no_grad()
def rank_users(user_emb: torch.Tensor, item_emb: torch.Tensor, users: torch.Tensor, rated: CSR,
               k: int, batch: Optional[int] = None, fused: bool = False,
               segments: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k (ids, scores) for each user id in ``users``: ``user_emb[u] @ item_emb.T``, rated
    items masked to -10e8, find_k_largest ordering. Returns device int32 / fp32 [len(users), k].

    ``batch`` users are scored per GEMM (default: a 4 GiB score buffer; the [B, d]·[d, I]
    product writes at 1.6 TB/s for B = 4,096 and 2.4 TB/s for B = 8,192 at the Yelp shape).
    ``fused=True`` takes :func:`rank_users_fused` instead (one kernel from the tables to the
    lists, no score matrix; ``segments`` is its item split): opt-in, because its scores differ
    from the library GEMM's in the last bits."""
    if fused:
        return rank_users_fused(user_emb, item_emb, users, rated, k, batch, segments)
    users = users.to(device=user_emb.device, dtype=torch.int64)
    n = users.numel()
    if batch is None:
        batch = max(1024, SCORE_BUFFER_BYTES // (4 * max(1, item_emb.shape[0])))
    out_ids = torch.empty((n, k), dtype=torch.int32, device=user_emb.device)
    out_sc = torch.empty((n, k), dtype=torch.float32, device=user_emb.device)
    it = item_emb.t().contiguous()
    for b0 in range(0, n, batch):
        ub = users[b0:b0 + batch]
        S = torch.mm(user_emb.index_select(0, ub), it)  # library GEMM (rocBLAS / hipBLASLt)
        mask_scores(S, rated, ub)
        ids, sc = topk_rows(S, k)
        out_ids[b0:b0 + batch] = ids
        out_sc[b0:b0 + batch] = sc
    return out_ids, out_sc


def ndcg_discount(k: int) -> List[float]:
    """1.0/math.log(n+2, 2) for n < k, as Metric.NDCG computes it (util/evaluation.py:92-95)."""
    return [1.0 / math.log(n + 2, 2) for n in range(k)]


class TestLists:
    """The test set of ``ranking_evaluation`` (``origin`` = data.test_set, util/evaluation.py:169)
    on the device: per test user (in the dict's order) the internal ids of its test items that
    exist in the training maps (sorted; items never seen in training can never be recommended,
    so they are never hits) and the full count ``len(origin[user])`` (the recall / hit-ratio /
    IDCG denominators count them)."""

    def __init__(self, origin: Dict, item_map: Dict, device):
        self.users = list(origin)
        counts = np.empty(len(self.users), dtype=np.int64)
        rowptr = np.zeros(len(self.users) + 1, dtype=np.int64)
        cols: List[np.ndarray] = []
        for r, u in enumerate(self.users):
            items = origin[u]
            counts[r] = len(items)
            ids = np.fromiter((item_map[i] for i in items if i in item_map), dtype=np.int64)
            ids.sort()
            cols.append(ids)
            rowptr[r + 1] = rowptr[r] + ids.size
        self.counts = counts
        self.rowptr = torch.from_numpy(rowptr).to(device)
        flat = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
        self.cols = torch.from_numpy(flat.astype(np.int32)).to(device)


@torch.no_grad()
def rank_metrics(ids: torch.Tensor, tests: TestLists, cutoffs: Sequence[int],
                 discount: Optional[torch.Tensor] = None) -> Tuple[np.ndarray, np.ndarray]:
    """hgd_rank_metrics: per test user and cut-off N, the distinct hits among ids[:, :N] and the
    DCG in position order (float64, bit-identical to Metric.NDCG's loop). ids: device int32
    [n_users, k] of internal item ids, rows in ``tests.users`` order."""
    if ids.dim() != 2 or ids.dtype != torch.int32 or ids.device.type != "cuda":
        raise TypeError("rank_metrics: ids must be a 2-D int32 device tensor")
    if ids.shape[0] != len(tests.users):
        raise ValueError(f"rank_metrics: {ids.shape[0]} lists for {len(tests.users)} test users")
    if ids.stride(1) != 1:
        ids = ids.contiguous()
    k = int(ids.shape[1])
    cut = [int(c) for c in cutoffs]
    if discount is None:
        discount = torch.tensor(ndcg_discount(k), dtype=torch.float64, device=ids.device)
    n = ids.shape[0]
    hits = torch.empty((n, len(cut)), dtype=torch.int32, device=ids.device)
    dcg = torch.empty((n, len(cut)), dtype=torch.float64, device=ids.device)
    carr = (ctypes.c_int32 * len(cut))(*cut)
    nat.check(nat.load().hgd_rank_metrics(
        ids.data_ptr(), n, ids.stride(0), k, tests.rowptr.data_ptr(),
        tests.cols.data_ptr() if tests.cols.numel() else None, carr, len(cut),
        discount.data_ptr(), hits.data_ptr(), dcg.data_ptr(),
        nat.stream_handle(ids.device)), "hgd_rank_metrics")
    return hits.cpu().numpy(), dcg.cpu().numpy()


def _seq_sum(values: np.ndarray) -> float:
    """Left-to-right float64 sum, as the reference's ``sum(list)`` / ``+=`` loops round it:
    ``np.cumsum`` accumulates sequentially (``np.sum`` is pairwise and Python >= 3.12's ``sum``
    compensated — both would round differently)."""
    return float(np.cumsum(np.asarray(values, dtype=np.float64))[-1]) if len(values) else 0.0


def ranking_evaluation(tests: TestLists, ids: torch.Tensor, N: Sequence[int]) -> List[str]:
    """Drop-in for ``ranking_evaluation(data.test_set, rec_list, N)`` (util/evaluation.py:169-196)
    when rec_list came from ``rank_users`` for ``tests.users``: the same list of strings
    ('Top N', 'Hit Ratio:…', 'Precision:…', 'Recall:…', 'NDCG:…' per N), the same float64
    arithmetic in the same order, from the device per-user hits / DCG."""
    N = [int(n) for n in N]
    order = sorted(set(N))
    hits, dcg = rank_metrics(ids, tests, order)
    disc = ndcg_discount(max(order))
    idcg_prefix = [0.0]  # IDCG of a c-item test list: the first min(N, c) discounts, in order
    for v in disc:
        idcg_prefix.append(idcg_prefix[-1] + v)
    idcg_prefix = np.asarray(idcg_prefix, dtype=np.float64)
    counts = tests.counts.astype(np.int64)
    total_num = int(counts.sum())  # Metric.hit_ratio (:17-29), integer
    n_users = len(counts)
    measure: List[str] = []
    for n in N:
        c = order.index(n)
        h = hits[:, c].astype(np.int64)
        hit_num = int(h.sum())
        hr = round(hit_num / total_num, 5)
        prec = round(hit_num / (n_users * n), 5)                                  # :49-52
        recall = round(_seq_sum(h / counts) / n_users, 5)                         # :54-58
        ndcg = round(_seq_sum(dcg[:, c] / idcg_prefix[np.minimum(counts, n)]) / n_users,
                     5)                                                           # :84-97
        measure.append('Top ' + str(n) + '\n')
        measure += ['Hit Ratio:' + str(hr) + '\n', 'Precision:' + str(prec) + '\n',
                    'Recall:' + str(recall) + '\n', 'NDCG:' + str(ndcg) + '\n']
    return measure


def evaluate_test_users(data, user_emb: torch.Tensor, item_emb: torch.Tensor,
                        topN: Sequence[int], tests: Optional[TestLists] = None,
                        rated: Optional[CSR] = None,
                        batch: Optional[int] = None,
                        fused: bool = False) -> Tuple[List[str], torch.Tensor, torch.Tensor]:
    """GraphRecommender.test() + ranking_evaluation (base/graph_recommender.py:61-92, 130-133)
    on the device up to the per-user counts: scores, masking, find_k_largest lists and the
    metric inputs. Returns (measure strings, ids, scores); ids / scores are the device
    [n_test_users, max(topN)] lists in data.test_set order (internal item ids)."""
    if tests is None:
        tests = TestLists(data.test_set, data.item, user_emb.device)
    if rated is None:
        rated = rated_csr(data.interaction_mat, user_emb.device)
    if not tests.users:
        raise ValueError("evaluate_test_users: empty test set")
    uid = torch.tensor([data.user[u] for u in tests.users], dtype=torch.int64)
    ids, sc = rank_users(user_emb, item_emb, uid, rated, max(int(n) for n in topN), batch,
                         fused=fused)
    return ranking_evaluation(tests, ids, topN), ids, sc


def test_rec_list(data, user_emb: torch.Tensor, item_emb: torch.Tensor, max_N: int,
                  batch: Optional[int] = None, fused: bool = False) -> Dict:
    """Drop-in for ``GraphRecommender.test()``: ``{user: [(item_name, score), ...]}`` over
    ``data.test_set`` in its iteration order, ready for the reference's ``evaluate()``."""
    users = list(data.test_set)
    if not users:
        return {}
    uid = torch.tensor([data.user[u] for u in users], dtype=torch.int64)
    rated = rated_csr(data.interaction_mat, user_emb.device)
    ids, sc = rank_users(user_emb, item_emb, uid, rated, max_N, batch, fused=fused)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    rec = {}
    for r, u in enumerate(users):
        rec[u] = [(data.id2item[int(i)], float(s)) for i, s in zip(ids[r], sc[r])]
    return rec
