"""Pairwise training batches, bit-identical to the reference's sampler, ≈11× faster per epoch.

``next_batch_pairwise(data, batch_size, n_negs=1, device=None)`` has the signature, outputs and
side effects of util/sampler.py:237-264 (paths relative to /root/reference/HD_SELFRec): it
shuffles ``data.training_data`` in place with Python's ``random.shuffle``, then per batch yields
``(u_idx, i_idx, j_idx)`` int64 tensors with ``n_negs`` negatives per record drawn by
``random.choice(list(data.item.keys()))`` and redrawn while in ``data.training_set_u[user]``.

The draws run in libhgd (``hgd_py_shuffle`` / ``hgd_sample_pairwise``: CPython's MT19937 and
``_randbelow`` restated in C++) on the state ``random.getstate()`` exposes, which is handed back
with ``random.setstate`` after every call — so the batches, the shuffled list and the Python
random stream afterwards are exactly those of the reference loop, including when the caller
stops early (each batch is drawn when it is requested, as the reference generator does).

``next_batch_unified(data, data_kg, batch_size, batch_size_kg, n_negs=1, device=None)`` is the
same for the KG carriers' generator (util/sampler.py:7-90), which also consumes NumPy's global
legacy ``RandomState`` (``hgd_py_shuffle_rows`` / ``hgd_sample_unified``); see its docstring.
"""
from __future__ import annotations

import ctypes
import operator
import random
from typing import Iterator, Tuple

import numpy as np
import torch

from . import _native as nat


def _mt_in() -> Tuple[tuple, np.ndarray]:
    st = random.getstate()
    return st, np.fromiter(st[1], dtype=np.uint32, count=len(st[1]))


def _mt_out(st: tuple, mt: np.ndarray) -> None:
    random.setstate((st[0], tuple(mt.tolist()), st[2]))


class _SamplerState:
    """Dense copies of ``data``'s training records and per-user item lists, plus the running
    permutation ``order`` of the ORIGINAL record list that the reference's repeated in-place
    shuffles produce (``data.training_data[k] is records[order[k]]``)."""

    def __init__(self, data):
        td = data.training_data
        self.records = list(td)
        n = len(td)
        self.order = np.arange(n, dtype=np.int64)
        self.rec_user = np.fromiter((data.user[r[0]] for r in td), dtype=np.int32, count=n)
        self.rec_item = np.fromiter((data.item[r[1]] for r in td), dtype=np.int32, count=n)
        self.n_users = len(data.user)
        self.n_items = len(data.item)
        # the user's training items (data.training_set_u[user]) as a sorted CSR of dense ids
        u = self.rec_user.astype(np.int64)
        i = self.rec_item.astype(np.int64)
        key = np.unique(u * max(self.n_items, 1) + i)
        uu = key // max(self.n_items, 1)
        self.items = (key % max(self.n_items, 1)).astype(np.int32)
        self.rowptr = np.zeros(self.n_users + 1, dtype=np.int64)
        np.add.at(self.rowptr, uu + 1, 1)
        np.cumsum(self.rowptr, out=self.rowptr)

    def matches(self, td) -> bool:
        n = len(self.records)
        if len(td) != n:
            return False
        return n == 0 or all(td[k] is self.records[self.order[k]] for k in {0, n // 2, n - 1})


def _state_of(data) -> _SamplerState:
    s = getattr(data, "_hgd_pairwise", None)
    if s is None or not s.matches(data.training_data):
        s = _SamplerState(data)
        data._hgd_pairwise = s
    return s


def next_batch_pairwise(data, batch_size: int, n_negs: int = 1,
                        device=None) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """Drop-in for util/sampler.py:237-264 (same batches, same in-place shuffle, same random
    state afterwards)."""
    lib = nat.load()
    s = _state_of(data)
    n = len(s.records)
    st, mt = _mt_in()
    nat.check(lib.hgd_py_shuffle(mt.ctypes.data, s.order.ctypes.data if n else None, n),
              "hgd_py_shuffle")
    _mt_out(st, mt)
    if n > 1:  # the reference shuffles the list itself
        data.training_data[:] = operator.itemgetter(*s.order.tolist())(s.records)
    ptr = 0
    while ptr < n:
        end = min(ptr + batch_size, n)
        b = end - ptr
        u = np.empty(b, dtype=np.int32)
        i = np.empty(b, dtype=np.int32)
        j = np.empty(max(b * n_negs, 1), dtype=np.int32)
        st, mt = _mt_in()
        nat.check(lib.hgd_sample_pairwise(
            mt.ctypes.data, s.order.ctypes.data, ptr, end, s.rec_user.ctypes.data,
            s.rec_item.ctypes.data, s.rowptr.ctypes.data,
            s.items.ctypes.data if s.items.size else None, s.n_users, s.n_items, int(n_negs),
            u.ctypes.data, i.ctypes.data, j.ctypes.data), "hgd_sample_pairwise")
        _mt_out(st, mt)
        ptr = end
        if device is not None and torch.device(device).type == "cuda":
            # one pinned staging block and one asynchronous copy: a pageable .to(device) waits
            # for the stream's queued work, which would stop the host from preparing the next
            # batch while the device still runs this one (segments start 16-byte aligned)
            s2 = b + (b & 1)
            host = torch.empty(2 * s2 + b * n_negs, dtype=torch.int64, pin_memory=True)
            hv = host.numpy()
            hv[:b], hv[s2:s2 + b], hv[2 * s2:] = u, i, j[:b * n_negs]
            dev = host.to(device, non_blocking=True)
            yield dev[:b], dev[s2:s2 + b], dev[2 * s2:]
            continue
        yield (torch.from_numpy(u.astype(np.int64)).to(device),
               torch.from_numpy(i.astype(np.int64)).to(device),
               torch.from_numpy(j[:b * n_negs].astype(np.int64)).to(device))


# ---- the unified CF + KG sampler (util/sampler.py:7-90) ------------------------------------
def _np_in() -> Tuple[tuple, np.ndarray]:
    st = np.random.get_state()
    mt = np.empty(625, dtype=np.uint32)
    mt[:624] = st[1]
    mt[624] = st[2]
    return st, mt


def _np_out(st: tuple, mt: np.ndarray) -> None:
    np.random.set_state((st[0], mt[:624].copy(), int(mt[624]), st[3], st[4]))


class _KgTables:
    """``train_kg_dict`` as a host CSR by head id: row ``h`` holds its (tail, relation) in list
    order. From a KnowledgeGraph it is one copy of its device CSR; from the reference's
    ``Knowledge`` one pass over the dict."""

    def __init__(self, data_kg):
        csr = getattr(data_kg, "train_kg", None)
        if csr is not None and hasattr(csr, "rowptr"):
            self.rowptr = csr.rowptr.cpu().numpy().astype(np.int64, copy=False)
            self.tail = csr.tail.cpu().numpy().astype(np.int64)
            self.rel = csr.rel.cpu().numpy().astype(np.int64)
            self.n_kg_train = int(data_kg.n_kg_train)
            self.key = None
            return
        d = data_kg.train_kg_dict
        self.key = (id(d), len(d))
        self.n_kg_train = len(data_kg.kg_train_data)
        heads = np.fromiter(d.keys(), dtype=np.int64, count=len(d))
        lens = np.fromiter((len(v) for v in d.values()), dtype=np.int64, count=len(d))
        if heads.size and heads.min() < 0:
            raise ValueError("next_batch_unified: negative head id in train_kg_dict")
        flat = np.array([p for v in d.values() for p in v], dtype=np.int64).reshape(-1, 2)
        n_rows = int(heads.max()) + 1 if heads.size else 1
        self.rowptr = np.zeros(n_rows + 1, dtype=np.int64)
        self.rowptr[heads + 1] = lens
        np.cumsum(self.rowptr, out=self.rowptr)
        # the dict's lists lie in key order in `flat`; move each to its head's row
        src = np.cumsum(lens) - lens
        pos = np.repeat(self.rowptr[heads] - src, lens) + np.arange(flat.shape[0])
        self.tail = np.empty(flat.shape[0], dtype=np.int64)
        self.rel = np.empty(flat.shape[0], dtype=np.int64)
        self.tail[pos] = flat[:, 0]
        self.rel[pos] = flat[:, 1]


def _tail_sets(kg: _KgTables) -> Tuple[np.ndarray, np.ndarray]:
    """``pos_tail_sets`` for every head id at once, as a CSR of ascending distinct tails; it does
    not depend on the epoch, so it is sorted once per table."""
    if not hasattr(kg, "set_rowptr"):
        n_rows = kg.rowptr.size - 1
        row = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(kg.rowptr))
        o = np.lexsort((kg.tail, row))
        row, tail = row[o], kg.tail[o]
        keep = np.ones(tail.size, dtype=bool)
        keep[1:] = (row[1:] != row[:-1]) | (tail[1:] != tail[:-1])
        kg.set_tail = np.ascontiguousarray(tail[keep])
        kg.set_rowptr = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(np.bincount(row[keep], minlength=n_rows), out=kg.set_rowptr[1:])
    return kg.set_rowptr, kg.set_tail


def _gather_rows(rowptr: np.ndarray, rows: np.ndarray, inside: np.ndarray):
    """(ptr, src, lens): the concatenation of CSR rows ``rows`` (empty where not ``inside``)
    takes element ``src[k]`` of the CSR's arrays at position k; ``ptr`` is its row pointer and
    ``lens`` its row lengths."""
    lo = np.where(inside, rowptr[rows], 0)
    lens = np.where(inside, rowptr[rows + 1] - lo, 0)
    ptr = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    src = np.repeat(lo - ptr[:-1], lens) + np.arange(int(ptr[-1]), dtype=np.int64)
    return ptr, src, lens


def _kg_tables(data_kg) -> _KgTables:
    t = getattr(data_kg, "_hgd_unified_kg", None)
    if t is not None and t.key is not None:
        d = data_kg.train_kg_dict
        if t.key != (id(d), len(d)):
            t = None
    if t is None:
        t = _KgTables(data_kg)
        try:
            data_kg._hgd_unified_kg = t
        except AttributeError:  # an object without a __dict__: rebuilt per epoch
            pass
    return t


def _raw_ids(s: _SamplerState) -> Tuple[np.ndarray, np.ndarray]:
    """Raw (user, item) ids of ``s.records`` (what ``np.array(data.training_data)`` holds)."""
    if not hasattr(s, "raw_user"):
        n = len(s.records)
        s.raw_user = np.fromiter((r[0] for r in s.records), dtype=np.int64, count=n)
        s.raw_item = np.fromiter((r[1] for r in s.records), dtype=np.int64, count=n)
    return s.raw_user, s.raw_item


def next_batch_unified(data, data_kg, batch_size: int, batch_size_kg: int, n_negs: int = 1,
                       device=None, head_ids: bool = False) -> Iterator[Tuple[torch.Tensor, ...]]:
    """Drop-in for util/sampler.py:7-90: per batch ``(u_idx, i_idx, j_idx, h_idx, r_idx,
    pos_t_idx, neg_t_idx)`` int64 tensors, the same batches as the reference and the same
    ``random`` and ``np.random`` (global legacy RandomState) states after any number of batches.

    ``data`` is the Interaction-like object (integer raw ids); ``data_kg`` is a
    :class:`~.ingest.KnowledgeGraph` or the reference's ``Knowledge`` (only ``train_kg_dict`` and
    ``len(kg_train_data)`` are read; a head missing from the dict has no triples, as its
    defaultdict gives).

    What is reproduced: the two epoch shuffles (``random.shuffle`` on 2-D arrays, whose row swap
    degenerates to ``x[i] = x[j]``: the CF records become a resample; of ``shuffle(kg_data)``
    only the draws), CPython's set order for the epoch's heads and ``all_tails`` (taken from
    CPython itself on integers of the same hashes), and per batch the CF negatives,
    ``np.random.randint(len(selected_kg_data), size=batch_size_kg)`` and the negative tails, in
    libhgd (``hgd_sample_unified``). ``data.training_data`` is untouched, as in the reference.
    Not reproduced: when ``kg_train_data.to_numpy()`` returns a view the reference scrambles
    ``data_kg.kg_train_data`` in place; nothing reads it afterwards, so it is left alone here.

    ``h_idx`` is the head's position in the epoch's head order (``h_dict[h]``, sampler.py:76);
    ``head_ids=True`` yields the head's entity id instead (what ``kg_loss`` indexes with). An
    empty selected-triple table raises ``ValueError`` like ``np.random.randint(0)``.
    """
    lib = nat.load()
    s = _state_of(data)
    kg = _kg_tables(data_kg)
    n = len(s.records)
    raw_u, raw_i = _raw_ids(s)
    # shuffle(kg_data): draws only; shuffle(cf_data): a resample of the current list order
    st, mt = _mt_in()
    nat.check(lib.hgd_py_shuffle_rows(mt.ctypes.data, None, kg.n_kg_train),
              "hgd_py_shuffle_rows(kg)")
    order = s.order.copy()
    nat.check(lib.hgd_py_shuffle_rows(mt.ctypes.data, order.ctypes.data if n else None, n),
              "hgd_py_shuffle_rows(cf)")
    _mt_out(st, mt)
    # the epoch's tables: CPython orders the two sets (equal ints and floats hash alike)
    heads_l = list(set(raw_u[order].tolist() + raw_i[order].tolist()))
    heads = np.array(heads_l, dtype=np.int64)
    n_heads = heads.size
    inside = (heads >= 0) & (heads < kg.rowptr.size - 1)
    hh = np.where(inside, heads, 0)
    sel_ptr, src, lens = _gather_rows(kg.rowptr, hh, inside)
    n_sel = int(sel_ptr[-1])
    sel_head = np.repeat(np.arange(n_heads, dtype=np.int64), lens)
    sel_tail = np.ascontiguousarray(kg.tail[src])
    sel_rel = np.ascontiguousarray(kg.rel[src])
    all_tails = np.array(list(set(sel_tail.tolist())), dtype=np.int64)
    # pos_tail_sets as a sorted CSR of distinct tails per head position
    set_rowptr, set_tail = _tail_sets(kg)
    tail_rowptr, src, _ = _gather_rows(set_rowptr, hh, inside)
    tail_sorted = np.ascontiguousarray(set_tail[src])
    rec_user = s.rec_user
    rec_item = s.rec_item
    bkg = int(batch_size_kg)
    cuda = device is not None and torch.device(device).type == "cuda"
    req = nat.UnifiedBatch()
    req.order, req.rec_user, req.rec_item = order.ctypes.data, rec_user.ctypes.data, \
        rec_item.ctypes.data
    req.user_rowptr = s.rowptr.ctypes.data
    req.user_items = s.items.ctypes.data if s.items.size else None
    req.n_users, req.n_items, req.n_negs = s.n_users, s.n_items, int(n_negs)
    req.sel_head, req.sel_rel, req.sel_tail = sel_head.ctypes.data, sel_rel.ctypes.data, \
        sel_tail.ctypes.data
    req.n_sel = n_sel
    req.head_ids = heads.ctypes.data if head_ids else None
    req.all_tails, req.n_tails = all_tails.ctypes.data, all_tails.size
    req.tail_rowptr, req.tail_sorted = tail_rowptr.ctypes.data, tail_sorted.ctypes.data
    req.n_heads, req.batch_kg = n_heads, bkg
    ptr = 0
    while ptr < n:
        end = min(ptr + batch_size, n)
        b = end - ptr
        if n_sel == 0:
            # the reference draws the CF negatives, then np.random.randint(0) raises
            u = np.empty(b, dtype=np.int32)
            j = np.empty(max(b * n_negs, 1), dtype=np.int32)
            st, mt = _mt_in()
            nat.check(lib.hgd_sample_pairwise(
                mt.ctypes.data, order.ctypes.data, ptr, end, rec_user.ctypes.data,
                rec_item.ctypes.data, s.rowptr.ctypes.data,
                s.items.ctypes.data if s.items.size else None, s.n_users, s.n_items,
                int(n_negs), u.ctypes.data, u.ctypes.data, j.ctypes.data), "hgd_sample_pairwise")
            _mt_out(st, mt)
            raise ValueError("high <= 0")
        # one block, segments 16-byte aligned; pinned when it goes to the device in one
        # asynchronous copy (see next_batch_pairwise)
        sizes = (b, b, b * n_negs, bkg, bkg, bkg, bkg)
        offs = [0]
        for z in sizes:
            offs.append(offs[-1] + z + (z & 1))
        host = torch.empty(max(offs[-1], 1), dtype=torch.int64, pin_memory=cuda)
        base = host.data_ptr()
        (req.out_u, req.out_i, req.out_j, req.out_h, req.out_r, req.out_t,
         req.out_n) = [base + 8 * o for o in offs[:7]]
        req.begin, req.end = ptr, end
        st, mt = _mt_in()
        nst, nmt = _np_in()
        req.py_state, req.np_state = mt.ctypes.data, nmt.ctypes.data
        status = lib.hgd_sample_unified(ctypes.byref(req))
        _mt_out(st, mt)
        _np_out(nst, nmt)
        nat.check(status, "hgd_sample_unified")
        ptr = end
        out = host.to(device, non_blocking=True) if cuda else host
        parts = tuple(out[o:o + z] for o, z in zip(offs, sizes))
        yield parts if cuda or device is None else tuple(p.to(device) for p in parts)
