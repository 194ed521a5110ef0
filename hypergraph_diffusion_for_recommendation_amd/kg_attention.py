"""KHGRec's knowledge-graph attention on the device (model/graph/KHGRec.py:298-331).

The reference's ``update_attention`` runs on every minibatch (KHGRec.py:122) with the batch's
8192 sampled triples: a loop over the relations (a ``torch.where``, two gathers and two matmuls
each, Equation 4), a COO build, a device → host → device round trip for
``torch.sparse.softmax(A_in.cpu(), dim=1)`` (Equation 5), and the result assigned to
``att_adj.data``. Here:

* :class:`KGAttentionPattern` is everything that depends on the indices only, built once per
  batch before the encoder has run: the relation-grouped order of the triples (for the score
  kernel) and the ``[n_entities, n_entities]`` attention matrix's CSR / CSC over ALL ``B``
  triples, sorted by (h, t, r) / (t, h, r).
* :meth:`KGAttentionPattern.update` is two launches, ``hgd_kg_attention_scores`` and
  ``hgd_kg_attention_softmax``, plus one 32-bit gather for the CSC-order values; it returns an
  ordinary :class:`~.incidence.Incidence` that every hop accepts.
* :func:`kg_attention` is the one-call form, the drop-in body of ``update_attention``.

``torch.sparse.softmax`` coalesces first: triples with the same (h, t) are summed before the
softmax, and batches are drawn with replacement, so duplicates are the normal case. Compacting
them would make the nonzero count data-dependent (a host read), so all ``B`` entries stay: the
first member of a run of equal (h, t) carries ``exp(s − m)/Z`` of the run's sum ``s`` and the others
carry exactly 0 — the same linear map at a fixed size. Inside a run the members stand in
relation order, equal triples in batch order: equal triples have bitwise equal scores, so a
run's sum — and with it every value — does not depend on the order the batch lists its triples
in. The triples of a relation disabled by ``relations`` are sorted behind the last row (the row
pointers end before them), so they take no part and a head left with none has an empty row.

Nothing here reads the device back, except the index check of ``validate=True``. No gradient
flows into the attention (the reference assigns ``.data``): ``update`` runs under ``no_grad`` on
a detached table.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .incidence import CSR, DEFAULT_SPLIT_CHUNK, Incidence, _gather32, _stream, _ws

__all__ = ["KGAttentionPattern", "kg_attention", "relation_mask"]


def _index_vector(x, name: str, what: str = "KGAttentionPattern") -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int64:
        raise TypeError(f"{what}: {name} must be an int64 LongTensor, got "
                        f"{getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() != 1:
        raise ValueError(f"{what}: {name} must be 1-D, got {tuple(x.shape)}")
    return x


def _check_tables(E, W, R, n_entities: int, n_relations: int):
    """dtype and shape checks of (ego_embed, trans_M, relation_emb); returns (d, dr)."""
    for x, name in ((E, "ego_embed"), (W, "trans_M"), (R, "relation_emb")):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"kg_attention: {name} must be a float32 tensor, got "
                            f"{getattr(x, 'dtype', type(x).__name__)}")
    if E.dim() != 2 or W.dim() != 3 or R.dim() != 2:
        raise ValueError(f"kg_attention: expected ego_embed [n, d], trans_M [r, d, dr], "
                         f"relation_emb [r, dr]; got {tuple(E.shape)}, {tuple(W.shape)}, "
                         f"{tuple(R.shape)}")
    d, dr = int(W.shape[1]), int(W.shape[2])
    if W.shape[0] != n_relations or R.shape[0] != n_relations:
        raise ValueError(f"kg_attention: trans_M / relation_emb hold {W.shape[0]} / "
                         f"{R.shape[0]} relations, expected {n_relations}")
    if tuple(E.shape) != (n_entities, d) or R.shape[1] != dr:
        raise ValueError(f"kg_attention: ego_embed {tuple(E.shape)} / relation_emb "
                         f"{tuple(R.shape)} do not match {n_entities} entities, d = {d}, "
                         f"dr = {dr}")
    if d == 0 or dr == 0:
        raise ValueError("kg_attention: d and dr must be > 0")
    return d, dr


def relation_mask(relations, n_relations: int, device) -> torch.Tensor:
    """uint8 [n_relations] on ``device``: 1 for the relation ids in ``relations`` (the reference's
    ``relations`` list; ids outside ``[0, n_relations)`` name no triple). A list or host tensor
    goes through one pinned buffer and an asynchronous copy; a device tensor of ids stays on the
    device; a uint8 / bool tensor of length ``n_relations`` already on ``device`` is taken as
    the mask itself. No host synchronisation either way."""
    device = torch.device(device)
    if isinstance(relations, torch.Tensor) and relations.dtype in (torch.uint8, torch.bool):
        if relations.shape != (n_relations,):
            raise ValueError(f"kg_attention: relation mask {tuple(relations.shape)} for "
                             f"{n_relations} relations")
        return relations.to(device=device, dtype=torch.uint8).contiguous()
    if isinstance(relations, torch.Tensor) and relations.is_cuda:
        ids = relations.reshape(-1).long()
        ok = (ids >= 0) & (ids < n_relations)
        cnt = torch.zeros(max(n_relations, 1), dtype=torch.int32, device=device)
        cnt.index_put_((ids.clamp(0, max(n_relations - 1, 0)),), ok.int(), accumulate=True)
        return (cnt[:n_relations] > 0).to(torch.uint8)
    ids = relations.tolist() if isinstance(relations, torch.Tensor) else list(relations)
    en = torch.zeros(n_relations, dtype=torch.uint8).pin_memory()
    for i in ids:
        if 0 <= int(i) < n_relations:
            en[int(i)] = 1
    return en.to(device, non_blocking=True)


def _sort(keys: torch.Tensor, n_keys: int):
    """hgd_sort_perm: (sorted keys, perm) of int32 keys in [0, n_keys), stable."""
    lib = nat.load()
    n = keys.numel()
    out = torch.empty_like(keys)
    perm = torch.empty_like(keys)
    if n:
        ws = _ws(lib.hgd_sort_perm_workspace_size(n), keys.device)
        nat.check(lib.hgd_sort_perm(keys.data_ptr(), n, n_keys, out.data_ptr(), perm.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream(keys.device)),
                  "hgd_sort_perm")
    return out, perm


def _rowptr(sorted_keys: torch.Tensor, n_rows: int) -> torch.Tensor:
    n = sorted_keys.numel()
    out = torch.empty(n_rows + 1, dtype=torch.int64, device=sorted_keys.device)
    nat.check(nat.load().hgd_rowptr_from_sorted(sorted_keys.data_ptr() if n else None, n, n_rows,
                                                out.data_ptr(), _stream(sorted_keys.device)),
              "hgd_rowptr_from_sorted")
    return out


class KGAttentionPattern:
    """The index-only half of ``update_attention`` for one batch of triples.

    ``h``, ``t``, ``r``: int64 ``LongTensor`` [B], as the sampler yields them (moved to the device
    of ``device`` or, by default, of ``h`` — which must then be a device tensor).
    ``relations``: the reference's ``relations`` argument, the relation ids that take part (None
    = all; ids outside ``[0, n_relations)`` name no triple, as in the reference's loop).
    ``validate``: read one error count back and raise ``ValueError`` on an index out of range —
    the one host read; with ``validate=False`` an out-of-range index is replaced by 0.

    Attributes (device tensors; int32 unless noted): ``h32`` / ``t32`` the narrowed ids in batch
    order; ``grp_perm`` / ``rel_off`` (int64 [n_relations+1]) the relation-grouped order;
    ``csr`` / ``csc`` the two orientations over all ``B`` entries; ``csr_perm`` entry → triple;
    ``perm_t`` CSC position → CSR position; ``rel_enable`` (uint8 [n_relations]) or None.
    """

    def __init__(self, h: torch.Tensor, t: torch.Tensor, r: torch.Tensor, n_entities: int,
                 n_relations: int, relations=None, validate: bool = True, device=None):
        h, t, r = _index_vector(h, "h"), _index_vector(t, "t"), _index_vector(r, "r")
        if not (h.numel() == t.numel() == r.numel()):
            raise ValueError(f"KGAttentionPattern: h, t, r differ in length "
                             f"({h.numel()}, {t.numel()}, {r.numel()})")
        n_entities, n_relations = int(n_entities), int(n_relations)
        B = int(h.numel())
        if n_entities < 0 or n_relations < 0 or n_entities >= 2 ** 31 - 1 or B >= 2 ** 31 - 1:
            raise ValueError("KGAttentionPattern: sizes must be in [0, 2^31 - 1)")
        if B and (n_entities == 0 or n_relations == 0):
            raise ValueError("KGAttentionPattern: triples without entities or relations")
        dev = torch.device(device) if device is not None else h.device
        if dev.type != "cuda":
            raise RuntimeError("KGAttentionPattern: needs a device (cuda/hip) target; there is "
                               "no CPU path")
        self.n_entities, self.n_relations, self.B, self.device = n_entities, n_relations, B, dev
        lib = nat.load()
        st = _stream(dev)

        def i32():
            return torch.empty(B, dtype=torch.int32, device=dev)

        self.h32, self.t32, r32 = i32(), i32(), i32()
        flags = torch.zeros(1, dtype=torch.int64, device=dev)
        if B:
            for src, upper, dst in ((h, n_entities, self.h32), (t, n_entities, self.t32),
                                    (r, n_relations, r32)):
                src = src.to(dev).contiguous()
                nat.check(lib.hgd_index_narrow(src.data_ptr(), B, upper, dst.data_ptr(),
                                               flags.data_ptr(), st), "hgd_index_narrow")
        if validate and B and int(flags.item()):
            raise ValueError(f"KGAttentionPattern: {int(flags.item())} indices out of range for "
                             f"{n_entities} entities / {n_relations} relations")
        self.rel_enable = None
        h_key, t_key = self.h32, self.t32
        if relations is not None:
            self.rel_enable = relation_mask(relations, n_relations, dev)
            if B:
                # a disabled relation's triples: the ghost row n_entities, behind every real one
                dead = self.rel_enable[r32.long()] == 0
                ghost = torch.full_like(self.h32, n_entities)
                h_key = torch.where(dead, ghost, self.h32)
                t_key = torch.where(dead, ghost, self.t32)
        # stable sorts by r, then t, then h: the (h, t, r) order, equal triples in batch order;
        # the first sort alone is the relation grouping of the score kernel
        r_sorted, self.grp_perm = _sort(r32, max(n_relations, 1))
        self.rel_off = _rowptr(r_sorted, n_relations)
        t_s, p2 = _sort(_gather32(t_key, self.grp_perm), n_entities + 1)
        p12 = _gather32(self.grp_perm, p2)
        h_s, p3 = _sort(_gather32(h_key, p12), n_entities + 1)
        self.csr_perm = _gather32(p12, p3)
        rowptr = _rowptr(h_s, n_entities)
        col = _gather32(self.t32, self.csr_perm)
        # CSC: a stable sort of the (ghosted) tails keeps (h, r) ascending inside each column
        tk_s, self.perm_t = _sort(_gather32(t_key, self.csr_perm), n_entities + 1)
        colptr = _rowptr(tk_s, n_entities)
        row_t = _gather32(_gather32(self.h32, self.csr_perm), self.perm_t)
        # no split plan (it would need a count on the host): a long row is walked by one lane
        # group, as in the capacity form of Incidence.drop
        self.csr = CSR(rowptr, col, n_entities, n_entities, 0, DEFAULT_SPLIT_CHUNK)
        self.csc = CSR(colptr, row_t, n_entities, n_entities, 0, DEFAULT_SPLIT_CHUNK)
        self.csr.configure_kernel()
        self.csc.configure_kernel()
        # never the ordered walk (incidence.spmm_row_order): its build is a sort of n_entities
        # keys per orientation per batch for B entries, and its gather permutation covers only
        # the rowptr[n] live entries, not the tail a `relations` filter leaves behind them
        self.csr.row_order_ok = self.csc.row_order_ok = False

    def group_first(self) -> torch.Tensor:
        """bool [B] in CSR order: the entry is the first of its run of equal (h, t) — the one
        that carries the run's softmax value (the kernel derives the same marks from ``col``)."""
        B = self.B
        first = torch.ones(B, dtype=torch.bool, device=self.device)
        if B > 1:
            rows = torch.repeat_interleave(
                torch.arange(self.n_entities + 1, device=self.device),
                torch.diff(torch.cat([self.csr.rowptr, torch.full_like(self.csr.rowptr[:1], B)])),
                output_size=B)
            col = self.csr.col
            first[1:] = (rows[1:] != rows[:-1]) | (col[1:] != col[:-1])
        return first

    def scores(self, ego_embed: torch.Tensor, trans_M: torch.Tensor,
               relation_emb: torch.Tensor) -> torch.Tensor:
        """Equation 4 for every triple, fp32 [B] in batch order (a disabled relation's entries
        are left unwritten)."""
        E, W, R = (x.detach() for x in (ego_embed, trans_M, relation_emb))
        d, dr = _check_tables(E, W, R, self.n_entities, self.n_relations)
        for x, name in ((E, "ego_embed"), (W, "trans_M"), (R, "relation_emb")):
            if x.device != self.device:
                raise RuntimeError(f"kg_attention: {name} is on {x.device}, the pattern on "
                                   f"{self.device}")
        if E.stride(1) != 1:
            E = E.contiguous()
        if R.stride(1) != 1:
            R = R.contiguous()
        W = W.contiguous()
        v = torch.empty(self.B, dtype=torch.float32, device=self.device)
        if self.B:
            nat.check(nat.load().hgd_kg_attention_scores(
                E.data_ptr(), E.stride(0), self.n_entities, W.data_ptr(), R.data_ptr(),
                R.stride(0), self.n_relations, d, dr, self.h32.data_ptr(), self.t32.data_ptr(),
                self.grp_perm.data_ptr(), self.rel_off.data_ptr(), nat.ptr(self.rel_enable),
                self.B, v.data_ptr(), _stream(self.device)), "hgd_kg_attention_scores")
        return v

    def softmax(self, v: torch.Tensor) -> Incidence:
        """Equation 5 over per-triple scores ``v`` (fp32 [B], batch order): the attention matrix
        as an :class:`Incidence` whose ``val`` / ``val_t`` are the row softmax in CSR / CSC
        order."""
        if v.dtype != torch.float32:
            raise TypeError(f"kg_attention: scores must be float32, got {v.dtype}")
        if v.shape != (self.B,):
            raise ValueError(f"kg_attention: {tuple(v.shape)} scores for {self.B} triples")
        v = v.detach().contiguous()
        dev = self.device
        lib = nat.load()
        val = torch.empty(self.B, dtype=torch.float32, device=dev)
        if self.B:
            wsb = lib.hgd_kg_attention_softmax_workspace_size(self.B)
            ws = _ws(wsb, dev)
            nat.check(lib.hgd_kg_attention_softmax(
                self.csr.rowptr.data_ptr(), self.csr.col.data_ptr(), self.csr_perm.data_ptr(),
                self.n_entities, self.B, v.data_ptr(), val.data_ptr(), ws.data_ptr(), wsb,
                _stream(dev)), "hgd_kg_attention_softmax")
        inc = Incidence(self.csr, self.csc, val, _gather32(val, self.perm_t))
        inc.perm_t = self.perm_t
        return inc

    @torch.no_grad()
    def update(self, ego_embed: torch.Tensor, trans_M: torch.Tensor,
               relation_emb: torch.Tensor) -> Incidence:
        """The attention matrix of this batch for the current embeddings (the value
        ``update_attention`` assigns to ``att_adj.data``, KHGRec.py:309-331)."""
        return self.softmax(self.scores(ego_embed, trans_M, relation_emb))


def kg_attention(ego_embed: torch.Tensor, h: torch.Tensor, t: torch.Tensor, r: torch.Tensor,
                 trans_M: torch.Tensor, relation_emb: torch.Tensor, n_entities: int,
                 relations=None, validate: bool = True) -> Incidence:
    """``update_attention(ego_embed, h, t, r, relations)`` (KHGRec.py:309-331) in one call: the
    row-softmaxed attention matrix ``[n_entities, n_entities]`` as an :class:`Incidence`."""
    n_relations = 0
    if isinstance(trans_M, torch.Tensor) and trans_M.dim():
        n_relations = int(trans_M.shape[0])
    _check_tables(ego_embed, trans_M, relation_emb, int(n_entities), n_relations)
    pattern = KGAttentionPattern(h, t, r, n_entities, n_relations, relations,
                                 validate=validate, device=ego_embed.device)
    return pattern.update(ego_embed, trans_M, relation_emb)
