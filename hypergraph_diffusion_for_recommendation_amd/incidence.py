"""Device-resident incidence structures for the propagation hops.

An :class:`Incidence` holds one sparse matrix ``A`` of shape ``[n_rows, n_cols]`` twice:

* ``csr``  — rows of ``A`` (the hop ``Y = A·X``, ``torch.sparse.mm(adj, X)``), and
* ``csc``  — rows of ``Aᵀ`` (the hop ``M = Aᵀ·X``, ``torch.sparse.mm(adj.t(), X)``),

plus the per-nonzero weights in both orders and cached degree scales. Everything is built on
the GPU by libhgd (``include/hgd.h``); this module only allocates buffers with the PyTorch
caching allocator and sequences the C-ABI calls. It replaces the per-call COO handling of the
reference (``base/torch_interface.py:8-12`` builds the COO; ``torch.sparse.mm`` coalesces it and
``HGCNConv`` rebuilds ``adj.t()`` on every call, ``model/graph/HGNN_HD4.py:459-462``).

Layout in HBM (N rows, E nonzeros): rowptr int64[N+1], col int32[E], val fp32[E] (optional),
for each orientation; split plans for rows longer than ``split_threshold`` nonzeros.
"""
from __future__ import annotations

import copy
import ctypes
import os
import weakref
from typing import Dict, Optional, Tuple

import torch

from . import _native as nat
from . import profiling

DEFAULT_SPLIT_THRESHOLD = 2048
DEFAULT_SPLIT_CHUNK = 512
SPLIT_THRESHOLD_MIN = 128
SPLIT_NNZ_PER_THRESHOLD = 8192
SEGMENTED_MAX_AVG_DEGREE = 32
# lane-group tasks needed to fill MI355X: 256 CUs × 16 waves × 4 groups of 16 lanes (d = 64)
TARGET_GROUPS = 16384
# the greedy row order's placement (hgd_row_order_greedy): the XCDs workgroups are dealt to
# round-robin on MI355X, and the chunks each XCD's part is cut into (1: the best order; more bound
# the host build)
ORDER_XCDS = 8
ORDER_CHUNKS_PER_XCD = 1
# the XCDs whose walkers pick their rows from one shared pool (hgd_row_order_greedy_pooled; 1: every
# XCD walks a part of its own; ORDER_XCDS: one pool of all rows, the most L2 hits and the longest
# build)
ORDER_XCDS_PER_POOL = 8


def order_pool_width() -> int:
    """The pool width a placed greedy order is built with: ``ORDER_XCDS_PER_POOL``, or what
    ``HGD_SPMM_ORDER_POOL`` (1, 2, 4 or 8) says. Read when an order is built, once per structure;
    not part of :func:`order_geometry` or of the key the orders are cached under."""
    env = os.environ.get("HGD_SPMM_ORDER_POOL", "")
    if env == "":
        return ORDER_XCDS_PER_POOL
    if env not in ("1", "2", "4", "8"):
        raise ValueError(f"HGD_SPMM_ORDER_POOL must be 1, 2, 4 or 8, got {env!r}")
    return int(env)


def auto_split(n_rows: int, nnz: int) -> Tuple[int, int]:
    """(threshold, chunk) for the long-row split. A row walked by one lane group costs ~1.4 µs
    per 16 nonzeros (dependent index → gather round trips), so one unsplit row of T nonzeros
    ends the hop no sooner than ~T/11 µs: large structures split rows above
    pow2_floor(nnz / 8192) nonzeros, clamped to [128, 2048], into chunks of half that (at most
    512) — the longest walk stays a fraction of the hop's streaming time. (A skewed catalogue's hop,
    scripts/bench_skewed_hop.py: 180 µs at 2048 / 512, 43 µs at 128 / 64; uniform graphs keep
    their rows whole — their degrees stay far below the threshold.) A structure with fewer
    rows than TARGET_GROUPS (e.g. ML-1M's 3,706 items × ~200 nonzeros) would leave most CUs idle
    with one group per row, so its rows are cut into chunks of ≈ nnz / TARGET_GROUPS nonzeros
    (power of two in [32, 512])."""
    if n_rows >= TARGET_GROUPS or nnz == 0:
        t = SPLIT_THRESHOLD_MIN
        while 2 * t <= nnz // SPLIT_NNZ_PER_THRESHOLD and t < DEFAULT_SPLIT_THRESHOLD:
            t *= 2
        return t, min(t // 2, DEFAULT_SPLIT_CHUNK)
    want = max(1, nnz // TARGET_GROUPS)
    chunk = 32
    while chunk < want and chunk < DEFAULT_SPLIT_CHUNK:
        chunk *= 2
    return 2 * chunk, chunk


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _stream(device) -> int:
    return nat.stream_handle(device)


_ORDER_GEOM: Dict[tuple, Tuple[int, int]] = {}


def order_geometry(d: int, blocked: bool, x_dtype: torch.dtype = torch.float32,
                   y_dtype: torch.dtype = torch.float32,
                   fused: bool = False) -> Tuple[int, int, int, int]:
    """``(window, rows_per_wg, n_xcd, chunks_per_xcd)`` of the greedy order for the hop at
    width ``d`` (``blocked``: the source-blocked hop): the first two from the launcher's own pass
    plan (hgd_spmm_order_geometry: 16 rows a workgroup and 16,384 gathers in an XCD's L2 at
    d = 64), the key the orders are cached under. ``x_dtype`` / ``y_dtype`` / ``fused``: the
    form of the hop when it is not the plain fp32 one (hgd_spmm_order_geometry_dt) — a 16-bit
    side has 8-column lanes and a 2·d-byte gathered piece, and the fused row epilogue walks a
    row wider than 128 columns in one pass. ``HGD_SPMM_ORDER_PLACE=0`` builds the same
    chunks as one sequence, not placed on the XCDs (a measurement switch; unset or ``1``:
    placed)."""
    env = os.environ.get("HGD_SPMM_ORDER_PLACE", "")
    if env not in ("", "0", "1"):
        raise ValueError(f"HGD_SPMM_ORDER_PLACE must be 0 or 1, got {env!r}")
    plain = x_dtype == torch.float32 and y_dtype == torch.float32 and not fused
    key = (int(d), bool(blocked)) + (() if plain else (x_dtype, y_dtype, bool(fused)))
    got = _ORDER_GEOM.get(key)
    if got is None:
        rows, window = ctypes.c_int32(0), ctypes.c_int64(0)
        if plain:
            ok = nat.load().hgd_spmm_order_geometry(int(d), int(bool(blocked)),
                                                    ctypes.byref(rows), ctypes.byref(window))
        else:
            ok = nat.load().hgd_spmm_order_geometry_dt(
                int(d), int(bool(blocked)), _HOP_DTYPES[x_dtype], _HOP_DTYPES[y_dtype],
                int(bool(fused)), ctypes.byref(rows), ctypes.byref(window))
        if not ok:
            raise ValueError(f"order_geometry: no pass plan at d = {d}")
        got = _ORDER_GEOM[key] = (int(window.value), int(rows.value))
    if env == "0":
        return got + (1, ORDER_XCDS * ORDER_CHUNKS_PER_XCD)
    return got + (ORDER_XCDS, ORDER_CHUNKS_PER_XCD)


def _need_geom(geom: Optional[tuple]) -> tuple:
    """A greedy order is one of a geometry: there is no default width to take one from."""
    if geom is None or len(geom) != 4:
        raise ValueError("a greedy order needs geom = order_geometry(d, blocked) of the hop it "
                         "is walked by")
    return tuple(int(g) for g in geom)


class CSR:
    """One orientation: ``rowptr`` int64 [n_rows+1], ``col`` int32 [nnz] (device tensors),
    and the long-row split plan used by :func:`spmm_csr`."""

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, n_rows: int, n_cols: int,
                 split_threshold: int = DEFAULT_SPLIT_THRESHOLD,
                 split_chunk: int = DEFAULT_SPLIT_CHUNK, plan_counts: Optional[Tuple] = None):
        self.rowptr = rowptr
        self.col = col
        self._ws_bytes: Dict[int, int] = {}  # hgd_spmm_workspace_size per width (spmm_csr)
        self.n_rows = int(n_rows)
        self.n_cols = int(n_cols)
        self.nnz = int(col.numel())
        self.device = rowptr.device
        self.split_threshold = int(split_threshold)
        self.split_chunk = int(split_chunk)
        # the columns of every row ascending (the CSC built by Incidence._from_sorted): required
        # by the source-blocked hop, whose block starts are binary searches inside each row
        self.cols_ascending = False
        self._col_blocks: Dict[int, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        self._blk_vals: Dict[Tuple[int, int], tuple] = {}
        self._col_block_plans: Dict[int, tuple] = {}
        self._blk_ws_bytes: Dict[Tuple[int, int], int] = {}
        self._col_blocks_ord: Dict[int, Tuple[torch.Tensor, ...]] = {}
        self._blk_ord_vals: Dict[Tuple[int, int], tuple] = {}
        self._packed: Dict[Tuple[int, int, int], tuple] = {}
        self._row_order: Optional[Tuple[torch.Tensor, ...]] = None
        # the greedy orders, by (block count or 0, window, rows per workgroup, XCDs, chunks)
        self._greedy: Dict[tuple, Tuple[torch.Tensor, ...]] = {}
        # whether the structure outlives the steps that hop over it (Incidence.persist): only
        # then is an order worth a build on the host. A structure made per step — an edge-dropped
        # one, a learned hypergraph's — keeps the min-column order, built on the stream
        self.persistent = False
        self._ord_vals: Dict[Tuple[int, int], tuple] = {}
        self._col_asc: Optional[torch.Tensor] = None
        self._plan_arrays = ()
        self.plan = nat.SplitPlan()
        self.plan.threshold = 0
        if plan_counts is not None:
            self._build_plan(*plan_counts)

    # -- split plan ---------------------------------------------------------------------
    def plan_count_async(self) -> Optional[torch.Tensor]:
        """Queues the (n_heavy, n_chunks) count; returns the device tensor to read later."""
        if self.split_threshold <= 0 or self.n_rows == 0 or self.nnz <= self.split_threshold:
            return None
        counts = torch.empty(2, dtype=torch.int64, device=self.device)
        nat.check(nat.load().hgd_split_plan_count(
            self.rowptr.data_ptr(), self.n_rows, self.split_threshold, self.split_chunk,
            counts.data_ptr(), _stream(self.device)), "hgd_split_plan_count")
        return counts

    def _build_plan(self, n_heavy: int, n_chunks: int) -> None:
        self._ws_bytes = {}
        n_heavy, n_chunks = int(n_heavy), int(n_chunks)
        if n_heavy == 0:
            self.plan.threshold = 0
            return
        dev = self.device
        heavy_rows = torch.empty(n_heavy, dtype=torch.int32, device=dev)
        heavy_cptr = torch.empty(n_heavy + 1, dtype=torch.int64, device=dev)
        chunk_heavy = torch.empty(n_chunks, dtype=torch.int32, device=dev)
        lib = nat.load()
        ws = _ws(lib.hgd_split_plan_workspace_size(self.n_rows), dev)
        nat.check(lib.hgd_split_plan_build(
            self.rowptr.data_ptr(), self.n_rows, self.split_threshold, self.split_chunk,
            heavy_rows.data_ptr(), heavy_cptr.data_ptr(), chunk_heavy.data_ptr(), n_heavy,
            n_chunks, ws.data_ptr(), ws.numel(), _stream(dev)), "hgd_split_plan_build")
        self._plan_arrays = (heavy_rows, heavy_cptr, chunk_heavy)
        p = self.plan
        p.threshold = self.split_threshold
        p.chunk = self.split_chunk
        p.n_heavy = n_heavy
        p.n_chunks = n_chunks
        p.heavy_rows = heavy_rows.data_ptr()
        p.heavy_cptr = heavy_cptr.data_ptr()
        p.chunk_heavy = chunk_heavy.data_ptr()

    def configure_kernel(self, segmented: Optional[bool] = None) -> None:
        """Selects the hop kernel: one row per lane group (default), or the segmented short-row
        walk (HGD_PLAN_SEGMENTED; only without split rows and for average degree below
        SEGMENTED_MAX_AVG_DEGREE). Measured on MI355X the segmented walk is 6 %
        faster on a Zipf item graph's user hop and 6 % slower on a uniform one, so it is opt-in:
        ``segmented=True`` or ``HGD_SEGMENTED=1`` in the environment."""
        env = os.environ.get("HGD_SEGMENTED")
        if segmented is None and env is not None:
            segmented = env == "1"
        if segmented is None:
            segmented = False
        short = (self.n_rows > 0 and self.nnz < SEGMENTED_MAX_AVG_DEGREE * self.n_rows)
        self.plan.flags = 1 if (segmented and short and self.n_heavy == 0) else 0
        self._ws_bytes = {}

    @property
    def segmented(self) -> bool:
        return bool(self.plan.flags & 1)

    def __deepcopy__(self, memo):
        # immutable device structure: copies of a module share it (the ctypes plan struct
        # holding raw device pointers cannot be pickled or duplicated meaningfully)
        return self

    def col_blocks(self, n_blocks: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The block-major copy of this structure for the source-blocked hop
        (hgd_spmm_col_blocks): ``(blk_start [n_blocks·n_rows+1] int64, blk_col [nnz] int32,
        blk_perm [nnz] int32)``, built once per block count on the current stream."""
        got = self._col_blocks.get(n_blocks)
        if got is None:
            if not self.cols_ascending:
                raise RuntimeError("col_blocks: the rows' columns are not known to be ascending")
            dev = self.device
            lib = nat.load()
            start = torch.empty(n_blocks * self.n_rows + 1, dtype=torch.int64, device=dev)
            bcol = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            perm = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            if self.n_rows:
                ws = _ws(lib.hgd_spmm_col_blocks_workspace_size(self.n_rows, n_blocks), dev)
                nat.check(lib.hgd_spmm_col_blocks(
                    self.rowptr.data_ptr(), self.col.data_ptr() if self.nnz else None,
                    self.n_rows, self.n_cols, n_blocks, start.data_ptr(),
                    bcol.data_ptr() if self.nnz else None, perm.data_ptr() if self.nnz else None,
                    ws.data_ptr(), ws.numel(), _stream(dev)), "hgd_spmm_col_blocks")
            else:
                start.zero_()
            got = self._col_blocks[n_blocks] = (start, bcol, perm)
        return got

    def ascending_col(self) -> torch.Tensor:
        """``col`` with every row's columns ascending (duplicates kept), as the fused ranking's
        binary search needs them: ``col`` itself when the rows are known to be ascending, else a
        copy sorted on the device by (row, column), built once and cached."""
        if self.cols_ascending or self.nnz == 0:
            return self.col
        if self._col_asc is None:
            rows = torch.repeat_interleave(
                torch.arange(self.n_rows, dtype=torch.int64, device=self.device),
                self.rowptr[1:] - self.rowptr[:-1], output_size=self.nnz)
            key = torch.sort(rows * max(1, self.n_cols) + self.col.to(torch.int64)).values
            self._col_asc = (key % max(1, self.n_cols)).to(torch.int32)
        return self._col_asc

    def blocked_values(self, n_blocks: int, val: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """``val`` (per-nonzero weights in this structure's order) gathered into the block-major
        order of :meth:`col_blocks`. Cached per tensor while it is alive and unmodified (its
        version counter), e.g. the cached ``Incidence.edge_values`` a training step passes to
        every hop; the last 8 are kept."""
        if val is None:
            return None
        return _gather32_cached(self._blk_vals, n_blocks, val, self.col_blocks(n_blocks)[2])

    def col_block_plans(self, n_blocks: int):
        """The split plans of the source blocks of :meth:`col_blocks`, for hgd_spmm_blocked_split:
        a ctypes array of ``n_blocks`` ``hgd_split_plan``, plan k built over block k's own CSR
        (``blk_start + k·n_rows``) with this structure's threshold and chunk — a row is heavy per
        block, so one of 5,000 nonzeros over 4 blocks may be light in all of them. The ``[P, 2]``
        (n_heavy, n_chunks) counts are read from the device once; the plans and their device
        arrays are cached per block count like the block-major copy."""
        got = self._col_block_plans.get(n_blocks)
        if got is None:
            start = self.col_blocks(n_blocks)[0]
            plans = (nat.SplitPlan * n_blocks)()
            arrays = []
            dev, lib, n = self.device, nat.load(), self.n_rows
            thr, chunk = int(self.plan.threshold), int(self.plan.chunk)
            if self.n_heavy and n:  # (without split rows no piece of a row is heavy either)
                st = _stream(dev)
                counts = torch.empty((n_blocks, 2), dtype=torch.int64, device=dev)
                for k in range(n_blocks):
                    nat.check(lib.hgd_split_plan_count(
                        start.data_ptr() + 8 * k * n, n, thr, chunk,
                        counts.data_ptr() + 16 * k, st), "hgd_split_plan_count")
                ws = _ws(lib.hgd_split_plan_workspace_size(n), dev)
                for k, (n_heavy, n_chunks) in enumerate(counts.tolist()):
                    if n_heavy == 0:
                        continue
                    heavy_rows = torch.empty(n_heavy, dtype=torch.int32, device=dev)
                    heavy_cptr = torch.empty(n_heavy + 1, dtype=torch.int64, device=dev)
                    chunk_heavy = torch.empty(n_chunks, dtype=torch.int32, device=dev)
                    nat.check(lib.hgd_split_plan_build(
                        start.data_ptr() + 8 * k * n, n, thr, chunk, heavy_rows.data_ptr(),
                        heavy_cptr.data_ptr(), chunk_heavy.data_ptr(), n_heavy, n_chunks,
                        ws.data_ptr(), ws.numel(), st), "hgd_split_plan_build")
                    arrays.append((heavy_rows, heavy_cptr, chunk_heavy))
                    p = plans[k]
                    p.threshold, p.chunk = thr, chunk
                    p.n_heavy, p.n_chunks = n_heavy, n_chunks
                    p.heavy_rows = heavy_rows.data_ptr()
                    p.heavy_cptr = heavy_cptr.data_ptr()
                    p.chunk_heavy = chunk_heavy.data_ptr()
            got = self._col_block_plans[n_blocks] = (plans, arrays)
        return got[0]

    def _greedy_order(self, n_blocks: int, geom: tuple) -> torch.Tensor:
        """The greedy order on the device: hgd_row_order_greedy (``n_blocks`` = 0) or
        hgd_col_block_order_greedy over a host copy of ``rowptr`` and ``col``, made for this
        build alone — a stream synchronisation, once per structure and geometry, outside any
        capture. A placed geometry (``n_xcd`` > 1) takes the pooled builders, the XCDs sharing
        pools :func:`order_pool_width` wide."""
        window, rows_per_wg, n_xcd, chunks = geom
        pool = order_pool_width() if n_xcd > 1 else 0
        if pool == 1 and chunks != 1:  # (parts cut into chunks: the builder that cuts them)
            pool = 0
        if pool and n_xcd % pool:
            raise ValueError(f"a pool of {pool} XCDs does not divide the geometry's {n_xcd}")
        rowptr, col = self.rowptr.cpu().contiguous(), self.col.cpu().contiguous()
        lib = nat.load()
        out = torch.empty(max(1, n_blocks) * self.n_rows, dtype=torch.int32)
        cp = col.data_ptr() if self.nnz else None
        name = ("hgd_col_block_order_greedy" if n_blocks else "hgd_row_order_greedy") + \
            ("_pooled" if pool else "")
        args = (rowptr.data_ptr(), cp, self.n_rows, self.n_cols) + \
            ((n_blocks,) if n_blocks else ()) + \
            (window, nat.ORDER_COL_CAP, rows_per_wg, n_xcd, pool if pool else chunks, 0,
             out.data_ptr())
        nat.check(getattr(lib, name)(*args), name)
        return out.to(self.device)

    def col_blocks_ordered(self, n_blocks: int, kind: int = nat.ORDER_MIN_COLUMN,
                           geom: Optional[tuple] = None) -> Tuple[torch.Tensor, ...]:
        """:meth:`col_blocks` with the rows of every source block in ascending order of their
        first column in that block, for hgd_spmm_blocked_ordered (hgd_spmm_col_blocks_ordered):
        ``(blk_start [n_blocks·n_rows+1] int64, blk_col [nnz] int32, blk_perm [nnz] int32,
        blk_out_row [n_blocks·n_rows] int32)`` — position p of block k holds row
        ``blk_out_row[k·n_rows + p]``. Built once per block count on the current stream.

        ``kind=ORDER_GREEDY``: every block in the greedy shared-column order for the hop whose
        ``geom`` is :func:`order_geometry` ``(d, True)``, which is then required
        (hgd_col_block_order_greedy on the host, then hgd_spmm_col_blocks_ordered_from): built
        once per block count and geometry, with a stream synchronisation."""
        if kind == nat.ORDER_GREEDY:
            return self._col_blocks_greedy(n_blocks, _need_geom(geom))
        got = self._col_blocks_ord.get(n_blocks)
        if got is None:
            if not self.cols_ascending:
                raise RuntimeError(
                    "col_blocks_ordered: the rows' columns are not known to be ascending")
            dev = self.device
            lib = nat.load()
            start = torch.empty(n_blocks * self.n_rows + 1, dtype=torch.int64, device=dev)
            bcol = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            perm = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            out_row = torch.empty(n_blocks * self.n_rows, dtype=torch.int32, device=dev)
            if self.n_rows:
                ws = _ws(lib.hgd_spmm_col_blocks_ordered_workspace_size(self.n_rows, n_blocks),
                         dev)
                nat.check(lib.hgd_spmm_col_blocks_ordered(
                    self.rowptr.data_ptr(), self.col.data_ptr() if self.nnz else None,
                    self.n_rows, self.n_cols, n_blocks, start.data_ptr(),
                    bcol.data_ptr() if self.nnz else None, perm.data_ptr() if self.nnz else None,
                    out_row.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                    "hgd_spmm_col_blocks_ordered")
            else:
                start.zero_()
            got = self._col_blocks_ord[n_blocks] = (start, bcol, perm, out_row)
        return got

    def _col_blocks_greedy(self, n_blocks: int, geom: tuple) -> Tuple[torch.Tensor, ...]:
        got = self._greedy.get((n_blocks,) + geom)
        if got is None:
            if not self.cols_ascending:
                raise RuntimeError(
                    "col_blocks_ordered: the rows' columns are not known to be ascending")
            dev = self.device
            lib = nat.load()
            start = torch.empty(n_blocks * self.n_rows + 1, dtype=torch.int64, device=dev)
            bcol = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            perm = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            out_row = self._greedy_order(n_blocks, geom)
            if self.n_rows:
                ws = _ws(lib.hgd_spmm_col_blocks_ordered_from_workspace_size(self.n_rows,
                                                                             n_blocks), dev)
                nat.check(lib.hgd_spmm_col_blocks_ordered_from(
                    out_row.data_ptr(), self.rowptr.data_ptr(),
                    self.col.data_ptr() if self.nnz else None, self.n_rows, self.n_cols, n_blocks,
                    start.data_ptr(), bcol.data_ptr() if self.nnz else None,
                    perm.data_ptr() if self.nnz else None, ws.data_ptr(), ws.numel(),
                    _stream(dev)), "hgd_spmm_col_blocks_ordered_from")
            else:
                start.zero_()
            got = self._greedy[(n_blocks,) + geom] = (start, bcol, perm, out_row)
        return got

    @staticmethod
    def _order_key(base, geom: Optional[tuple]):
        """The cache key of what is gathered through an order: ``base`` for the min-column order
        (``geom`` None), with the geometry beside it for a greedy one."""
        return base if geom is None else (base,) + tuple(geom)

    def _blocks_of(self, n_blocks: int, geom: Optional[tuple]):
        return (self.col_blocks_ordered(n_blocks) if geom is None
                else self._col_blocks_greedy(n_blocks, geom))

    def blocked_ordered_values(self, n_blocks: int, val: Optional[torch.Tensor],
                               geom: Optional[tuple] = None) -> Optional[torch.Tensor]:
        """``val`` (per-nonzero weights) in the entry order of :meth:`col_blocks_ordered` (with
        ``geom``: of the greedy order of that geometry); cached like :meth:`blocked_values`."""
        if val is None:
            return None
        return _gather32_cached(self._blk_ord_vals, self._order_key(2 * n_blocks, geom), val,
                                self._blocks_of(n_blocks, geom)[2])

    def blocked_ordered_scale(self, n_blocks: int, row_scale: Optional[torch.Tensor],
                              geom: Optional[tuple] = None) -> Optional[torch.Tensor]:
        """``row_scale`` (one per row) as ``[n_blocks·n_rows]`` in the processing order of
        :meth:`col_blocks_ordered` (with ``geom``: of the greedy order of that geometry); cached
        like :meth:`blocked_values`."""
        if row_scale is None:
            return None
        return _gather32_cached(self._blk_ord_vals, self._order_key(2 * n_blocks + 1, geom),
                                row_scale, self._blocks_of(n_blocks, geom)[3])

    def packed_entries(self, n_blocks: int, src_scale: torch.Tensor,
                       idx_bits: int = nat.PACKED_IDX_BITS,
                       geom: Optional[tuple] = None) -> Optional[tuple]:
        """The entries of :meth:`col_blocks_ordered` packed for hgd_spmm_blocked_packed, for
        per-nonzero weights that are ``src_scale[col]`` (a float32 scale over this structure's
        ``n_cols`` source rows): ``(ent [nnz] int32 bits, dict [n_dict] float32, n_dict)`` with
        ``ent = (col − first source row of the block) | code << idx_bits`` and ``dict[code]`` the
        weight — the distinct values of ``src_scale`` by bit pattern, so ``dict[code of c]`` is
        ``src_scale[c]`` bit for bit. ``None`` when a block has more than ``2^idx_bits`` source
        rows or the scale too many distinct values (hgd_spmm_packed_fits). The dictionary size is
        read from the device once per scale tensor; the result is cached per (block count, bits,
        tensor) while the tensor is alive and unmodified, like :meth:`blocked_values`, so the
        weight copy of :meth:`blocked_ordered_values` is never built on this path."""
        try:
            version = src_scale._version
        except RuntimeError:  # an inference tensor tracks no version: built every call
            version = None
        key = (self._order_key(n_blocks, geom), idx_bits, id(src_scale))
        hit = self._packed.get(key)
        if (hit is not None and version is not None and hit[0]() is src_scale
                and hit[1] == version):
            return hit[2]
        if src_scale.dtype != torch.float32 or src_scale.numel() != self.n_cols:
            raise ValueError("packed_entries: src_scale must be float32 [n_cols]")
        lib = nat.load()
        bits, code = torch.unique(src_scale.contiguous().view(torch.int32), return_inverse=True)
        n_dict = int(bits.numel())
        got = None
        if lib.hgd_spmm_packed_fits(self.n_cols, n_blocks, n_dict, idx_bits):
            start, bcol, _, _ = self._blocks_of(n_blocks, geom)
            code = code.to(torch.int32)
            ent = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
            nat.check(lib.hgd_spmm_pack_entries(
                start.data_ptr(), bcol.data_ptr(), code.data_ptr(), self.n_rows, self.n_cols,
                self.nnz, n_blocks, n_dict, idx_bits, ent.data_ptr(), _stream(self.device)),
                "hgd_spmm_pack_entries")
            got = (ent, bits.view(torch.float32), n_dict)
        if len(self._packed) >= 8:
            self._packed.pop(next(iter(self._packed)))
        self._packed[key] = (weakref.ref(src_scale), version, got)
        return got

    def row_order(self, kind: int = nat.ORDER_MIN_COLUMN, geom: Optional[tuple] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The rows in ascending order of their smallest column, for the ordered hop
        (hgd_spmm_row_order): ``(order [n_rows] int32, rowptr_o [n_rows+1] int64, col_o [nnz]
        int32, perm [nnz] int32)`` — position p processes row ``order[p]``, whose nonzeros are
        ``[rowptr_o[p], rowptr_o[p+1])`` of ``col_o`` in their own order; ``perm`` is the source
        position of every entry. Built once, on the current stream.

        ``kind=ORDER_GREEDY``: the greedy shared-column order for the hop whose ``geom`` is
        :func:`order_geometry` ``(d, False)``, which is then required (hgd_row_order_greedy on the
        host, then hgd_spmm_row_order_from): built once per geometry, with a stream
        synchronisation."""
        if kind == nat.ORDER_GREEDY:
            return self._row_order_greedy(_need_geom(geom))
        got = self._row_order
        if got is None:
            dev = self.device
            lib = nat.load()
            order = torch.empty(self.n_rows, dtype=torch.int32, device=dev)
            rowptr_o = torch.empty(self.n_rows + 1, dtype=torch.int64, device=dev)
            col_o = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            perm = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            if self.n_rows:
                ws = _ws(lib.hgd_spmm_row_order_workspace_size(self.n_rows), dev)
                nat.check(lib.hgd_spmm_row_order(
                    self.rowptr.data_ptr(), self.col.data_ptr() if self.nnz else None,
                    self.n_rows, self.n_cols, order.data_ptr(), rowptr_o.data_ptr(),
                    col_o.data_ptr() if self.nnz else None, perm.data_ptr() if self.nnz else None,
                    ws.data_ptr(), ws.numel(), _stream(dev)), "hgd_spmm_row_order")
            else:
                rowptr_o.zero_()
            got = self._row_order = (order, rowptr_o, col_o, perm)
        return got

    def _row_order_greedy(self, geom: tuple) -> Tuple[torch.Tensor, ...]:
        got = self._greedy.get((0,) + geom)
        if got is None:
            dev = self.device
            lib = nat.load()
            rowptr_o = torch.empty(self.n_rows + 1, dtype=torch.int64, device=dev)
            col_o = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            perm = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            order = self._greedy_order(0, geom)
            if self.n_rows:
                ws = _ws(lib.hgd_spmm_row_order_from_workspace_size(self.n_rows), dev)
                nat.check(lib.hgd_spmm_row_order_from(
                    order.data_ptr(), self.rowptr.data_ptr(),
                    self.col.data_ptr() if self.nnz else None, self.n_rows, self.n_cols,
                    rowptr_o.data_ptr(), col_o.data_ptr() if self.nnz else None,
                    perm.data_ptr() if self.nnz else None, ws.data_ptr(), ws.numel(),
                    _stream(dev)), "hgd_spmm_row_order_from")
            else:
                rowptr_o.zero_()
            got = self._greedy[(0,) + geom] = (order, rowptr_o, col_o, perm)
        return got

    def _rows_of(self, geom: Optional[tuple]):
        return self.row_order() if geom is None else self._row_order_greedy(geom)

    def ordered_values(self, val: Optional[torch.Tensor],
                       geom: Optional[tuple] = None) -> Optional[torch.Tensor]:
        """``val`` (per-nonzero weights) in the entry order of :meth:`row_order` (with ``geom``:
        of the greedy order of that geometry); cached like :meth:`blocked_values`."""
        if val is None:
            return None
        return _gather32_cached(self._ord_vals, self._order_key(0, geom), val,
                                self._rows_of(geom)[3])

    def ordered_scale(self, row_scale: Optional[torch.Tensor],
                      geom: Optional[tuple] = None) -> Optional[torch.Tensor]:
        """``row_scale`` (one per row) in the processing order of :meth:`row_order` (with
        ``geom``: of the greedy order of that geometry); cached like :meth:`blocked_values`."""
        if row_scale is None:
            return None
        return _gather32_cached(self._ord_vals, self._order_key(1, geom), row_scale,
                                self._rows_of(geom)[0])

    def order_source(self) -> "CSR":
        """The structure whose row orders, ordered weights and ordered scales this one's hops
        walk: itself, or for an edge-dropped view (:meth:`Incidence.masked`) its parent — a view
        is made on every step, and what depends on the structure alone is built once per
        structure, not once per step."""
        return getattr(self, "_order_parent", None) or self

    def ordered_mask(self, geom: Optional[tuple] = None) -> torch.Tensor:
        """An edge-dropped view's ``mask`` in the entry order of its :meth:`order_source`'s
        :meth:`row_order` (with ``geom``: of the greedy order of that geometry): one
        hgd_gather_u8 through the order's ``perm``, on the current stream, cached on the view
        per order — the view's own per-step cost of an ordered hop."""
        cache = self.__dict__.setdefault("_mask_ord", {})
        key = self._order_key(0, geom)
        got = cache.get(key)
        if got is None:
            perm = self.order_source()._rows_of(geom)[3]
            got = torch.empty_like(self.mask)
            if self.nnz:
                nat.check(nat.load().hgd_gather_u8(
                    self.mask.data_ptr(), perm.data_ptr(), self.nnz, got.data_ptr(),
                    _stream(self.device)), "hgd_gather_u8")
            cache[key] = got
        return got

    @property
    def n_heavy(self) -> int:
        return int(self.plan.n_heavy) if self.plan.threshold > 0 else 0

    def degrees(self) -> torch.Tensor:
        return self.rowptr[1:] - self.rowptr[:-1]


def spmm_blocks(csr: CSR, d: int, x_dtype: torch.dtype = torch.float32) -> int:
    """How many source blocks the hop over ``csr`` at width ``d`` gathering a table of
    ``x_dtype`` runs in (0 = one pass).

    The hop gathers one d-wide row of X per nonzero at random. When X is small enough for the
    256 MB Infinity Cache (the item table a hop into users reads: 256 MB at d = 64) the gathers
    run at ~7.5 TB/s; a larger table (the 2.56 GB user table the hop into items reads) runs at the
    random-gather rate of HBM, ~5.9 TB/s. hgd_spmm_blocked cuts the source rows into P ranges
    and sums a row's nonzeros of one range per pass, so each pass gathers from a slice 1/P as
    large, for P−1 extra read+write passes over Y. Measured on MI355X at 10 M users × 1 M items
    × 100 M edges (scripts/bench_mall_blocked.py): d = 64 −13 % at P = 4,
    d = 128 −7 % at P = 8, d = 32 −4 % at P = 4 (−1 % at P = 2); hence about one block per
    640 MiB of the table a pass gathers from, at least 4, from 1 GiB. Between 512 MiB and 1 GiB
    two blocks: the 32-column slices of a 5 M-user shard (the sharded hop at N = 2, 640 MB)
    −4 % at P = 2; a 320 MB table (N = 4) is 3 % slower blocked. A blocked hop runs rows wider
    than 128 as 128-column passes (d = 256: −6 % at P = 8; in the plain hop's 64-column passes
    blocking gained nothing, 256 B gathered from every 1 KB row).

    Only for a structure whose rows' columns ascend (the CSC of an Incidence), without split
    rows or the segmented walk. ``HGD_SPMM_BLOCKS``: ``0`` turns it off, an integer P forces P
    blocks (1 = off) wherever it applies, a 16-bit hop (hgd_spmm_blocked_dt) included, unset =
    the size rule. The rule is by the table's element type (hgd_spmm_blocks_for_dt): the
    constants above were measured over 4-byte rows; over a bfloat16 table no block count beat
    the plain hop at the same shapes (d = 64: 2.83 ms plain, 2.88 at P = 2, 3.05 at P = 4;
    DESIGN.md §4.1), so the rule never blocks one."""
    if x_dtype not in _HOP_DTYPES:
        raise TypeError(f"spmm_blocks: x_dtype must be float32 or bfloat16, got {x_dtype}")
    if not csr.cols_ascending or csr.n_heavy or csr.segmented or csr.nnz == 0:
        return 0
    if getattr(csr, "mask", None) is not None:
        return 0  # an edge-dropped view's hop is the masked kernel: spmm_csr never blocks it
    env = os.environ.get("HGD_SPMM_BLOCKS", "")
    if env not in ("", "auto"):
        p = int(env)
        if p < 0 or p > 64:
            raise ValueError(f"HGD_SPMM_BLOCKS must be 0..64, got {env!r}")
        return p if p > 1 else 0
    # the library's size rule (hgd_spmm_blocks_for_dt; for a float32 table hgd_spmm_blocks_for's,
    # which the native incidence objects share)
    return int(nat.load().hgd_spmm_blocks_for_dt(csr.n_cols, int(d), _HOP_DTYPES[x_dtype]))


def spmm_blocks_split(csr: CSR, d: int, x_dtype: torch.dtype = torch.float32) -> int:
    """How many source blocks the fp32 hop over ``csr``, a structure WITH split rows, runs in at
    width ``d`` (0 = the plain split hop, hgd_spmm with the structure's plan).

    :func:`spmm_blocks` answers 0 for every structure with split rows, i.e. for every skewed
    catalogue; this is the question it leaves open. hgd_spmm_blocked_split runs the blocks of
    :meth:`CSR.col_blocks` each under its own split plan (:meth:`CSR.col_block_plans`): a row
    is heavy per block, the chunk partials of one block at a time live in one workspace, and Y
    is written once per row and block.

    Only for a structure with split rows whose rows' columns ascend, without a mask or the
    segmented flag, gathering a float32 table (into a float32 output: spmm_csr asks for no other).
    ``HGD_SPMM_BLOCKS_SPLIT``: ``0`` off, an integer P in 2..64 forces P blocks wherever it
    applies, unset (or ``auto``) = the library's rule (hgd_spmm_blocks_split_for, DESIGN.md
    §4.1). ``HGD_SPMM_BLOCKS`` has no say here, nor this variable in :func:`spmm_blocks`."""
    if x_dtype not in _HOP_DTYPES:
        raise TypeError(f"spmm_blocks_split: x_dtype must be float32 or bfloat16, got {x_dtype}")
    if x_dtype != torch.float32 or not csr.n_heavy:
        return 0
    if not csr.cols_ascending or csr.segmented or csr.nnz == 0:
        return 0
    if getattr(csr, "mask", None) is not None:
        return 0
    env = os.environ.get("HGD_SPMM_BLOCKS_SPLIT", "")
    if env not in ("", "auto"):
        p = int(env)
        if p != 0 and not 2 <= p <= 64:
            raise ValueError(f"HGD_SPMM_BLOCKS_SPLIT must be 0 or 2..64, got {env!r}")
        return p
    return int(nat.load().hgd_spmm_blocks_split_for(
        csr.n_cols, int(d), csr.nnz, int(csr.plan.n_chunks), int(csr.plan.chunk)))


def spmm_row_order(csr: CSR, d: int, x_dtype: torch.dtype = torch.float32,
                   y_dtype: torch.dtype = torch.float32, fused: bool = False,
                   masked: bool = False) -> bool:
    """Whether the hop over ``csr`` at width ``d`` walks its rows in an order of its
    own (hgd_spmm_ordered over :meth:`CSR.row_order`): ascending smallest column, or the greedy
    shared-column order — which of the two is :func:`spmm_order_kind`'s answer. Without the
    keyword arguments the question is the plain fp32 hop's; ``x_dtype`` / ``y_dtype`` (a
    bfloat16 table or output), ``fused`` (a fused row epilogue) and ``masked`` (an edge-dropped
    view) ask it of the other forms, whose entry points are the ordered twins of their own
    (hgd_spmm_fused_ordered, hgd_spmm_masked_ordered, hgd_spmm_ordered_dt, ...) and whose rule
    is hgd_spmm_row_order_for_dt, set per form by measurement.

    A short row's gathers are spread over the whole source table, so an XCD's 4 MiB of L2 sees
    almost no reuse; rows that share their smallest column processed next to each other make
    the first gather of most rows an L2 hit (the greedy order: a fifth of all gathers). Nothing
    inside a row changes: the sums are bitwise
    those of hgd_spmm. The price is Y rows written in permuted order and one 4-byte row id per
    row. The size rule is the library's (hgd_spmm_row_order_for).

    Only without split rows or the segmented walk. ``HGD_SPMM_ROW_ORDER``: ``0`` off, ``1`` on
    wherever it applies, unset (or ``auto``) = the size rule."""
    if csr.n_heavy or csr.segmented or csr.nnz == 0:
        return False
    if not getattr(csr, "row_order_ok", True):
        # a structure that opted out (a KG attention pattern: rebuilt per batch, few entries in
        # many rows, and its arrays may run past rowptr[n_rows], which the order's gather
        # permutation does not cover) — not even when the environment forces the order
        return False
    env = os.environ.get("HGD_SPMM_ROW_ORDER", "")
    if env not in ("", "auto"):
        if env not in ("0", "1"):
            raise ValueError(f"HGD_SPMM_ROW_ORDER must be 0 or 1, got {env!r}")
        return env == "1"
    if x_dtype == torch.float32 and y_dtype == torch.float32 and not fused and not masked:
        return bool(nat.load().hgd_spmm_row_order_for(csr.n_rows, csr.n_cols, csr.nnz, int(d)))
    return bool(nat.load().hgd_spmm_row_order_for_dt(
        csr.n_rows, csr.n_cols, csr.nnz, int(d), _HOP_DTYPES[x_dtype], _HOP_DTYPES[y_dtype],
        int(bool(fused)), int(bool(masked))))


def spmm_block_order(csr: CSR, d: int, blocks: int) -> bool:
    """Whether the fp32 source-blocked hop over ``csr`` at width ``d`` in ``blocks`` blocks
    walks each block's rows in an order of the block's own (hgd_spmm_blocked_ordered over
    :meth:`CSR.col_blocks_ordered`): ascending first column in that block, or the block's greedy
    shared-column order — which of the two is :func:`spmm_order_kind`'s answer.

    :func:`spmm_row_order`'s idea inside one source block: a row piece of ~25 nonzeros gathers
    from the whole slice of the block, so pieces that share their first column processed next to
    each other make that gather an L2 hit. Each piece's sum and the order of the blocks are
    unchanged: Y is bitwise hgd_spmm_blocked's. The price is one 4-byte row id per row and
    block, and the row scale gathered per block. The size rule is the library's
    (hgd_spmm_block_order_for).

    ``HGD_SPMM_BLOCK_ORDER``: ``0`` off, ``1`` on wherever the hop runs blocked, unset (or
    ``auto``) = the size rule."""
    if blocks <= 1 or csr.nnz == 0:
        return False
    env = os.environ.get("HGD_SPMM_BLOCK_ORDER", "")
    if env not in ("", "auto"):
        if env not in ("0", "1"):
            raise ValueError(f"HGD_SPMM_BLOCK_ORDER must be 0 or 1, got {env!r}")
        return env == "1"
    return bool(nat.load().hgd_spmm_block_order_for(csr.n_rows, csr.n_cols, csr.nnz, int(d),
                                                    int(blocks)))


def spmm_order_kind(csr: CSR, d: int, blocks: int = 0) -> int:
    """Which order an ordered fp32 hop over ``csr`` at width ``d`` walks (``blocks`` > 1: each
    source block of the blocked hop), for a hop :func:`spmm_row_order` / :func:`spmm_block_order`
    has turned on: ``ORDER_MIN_COLUMN`` or ``ORDER_GREEDY``.

    The greedy order picks the next row by how many of its columns the XCD's L2 still holds, and
    gives every XCD a contiguous part of the rows (hgd_row_order_greedy); it is
    built on the host from a copy of the structure, once, with a stream synchronisation. Y is
    bitwise the same under either. The rule is the library's (hgd_spmm_row_order_kind_for):
    greedy wherever the size rules order the hop; a hop ordered only because the environment
    forces it walks the min-column order, whose build stays on the stream.

    Only for a structure that persists (``csr.persistent``, set by :meth:`Incidence.persist`: a
    :class:`ShardedIncidence` says it of its graph). Every other structure — the edge-dropped
    incidences :meth:`Incidence.drop` makes on every training step, possibly inside a captured
    step, a learned hypergraph's — walks the min-column order whatever the rule and the
    environment say: the greedy build copies the structure to the host and synchronises the
    stream, which a step can neither afford nor, captured, do.

    ``HGD_SPMM_ORDER_KIND``: ``1`` min column, ``2`` greedy wherever a hop is ordered, unset (or
    ``auto``) = the rule. (``HGD_SPMM_ROW_ORDER`` / ``HGD_SPMM_BLOCK_ORDER`` stay the 0 / 1
    switches of whether a hop is ordered at all.)"""
    env = os.environ.get("HGD_SPMM_ORDER_KIND", "")
    if env not in ("", "auto"):
        if env not in ("1", "2"):
            raise ValueError(f"HGD_SPMM_ORDER_KIND must be 1 or 2, got {env!r}")
    if not getattr(csr, "persistent", False):
        # made per step (Incidence.drop, a learned hypergraph, ...) or never said to last: the
        # greedy build — a host copy, seconds of host work, a stream synchronisation that cannot
        # run inside a capture — would be paid by every step. Not even when the environment
        # forces it
        return nat.ORDER_MIN_COLUMN
    if env not in ("", "auto"):
        return int(env)
    kind = nat.load().hgd_spmm_row_order_kind_for(csr.n_rows, csr.n_cols, csr.nnz, int(d),
                                                  int(blocks))
    return nat.ORDER_GREEDY if kind == nat.ORDER_GREEDY else nat.ORDER_MIN_COLUMN


def spmm_packed(csr: CSR, blocks: int, src_scale: Optional[torch.Tensor],
                geom: Optional[tuple] = None) -> Optional[tuple]:
    """The packed entries the fp32 block-ordered hop over ``csr`` in ``blocks`` blocks runs on
    (hgd_spmm_blocked_packed over :meth:`CSR.packed_entries`), or ``None`` for the weighted hop.

    When the weights are a scale over the source rows expanded per nonzero (``src_scale``: the
    degree scales of a binary incidence, a few dozen distinct values), a nonzero is one word —
    its column inside the block and a 10-bit code of its weight — instead of a column and a
    weight: half the streamed index bytes, the same fmaf chains, Y bitwise
    hgd_spmm_blocked_ordered's. It fits (hgd_spmm_packed_fits) when every block is within 2^22
    source rows and the scale has at most 1024 distinct values; the rule is the library's
    (hgd_spmm_packed_for): it fits and the blocks are as large as the size rules
    make them, at least 65,536 source rows each.

    ``HGD_SPMM_PACKED``: ``0`` off, ``1`` on wherever it fits, unset (or ``auto``) = the rule."""
    if blocks <= 1 or csr.nnz == 0:
        return None
    env = os.environ.get("HGD_SPMM_PACKED", "")
    if env not in ("", "auto", "0", "1"):
        raise ValueError(f"HGD_SPMM_PACKED must be 0 or 1, got {env!r}")
    rule = nat.load().hgd_spmm_packed_for
    if env == "0" or src_scale is None:
        return None
    if env != "1" and not rule(csr.n_cols, int(blocks), 1, nat.PACKED_IDX_BITS):
        return None  # (not even with one weight: the scale's are not counted for nothing)
    got = csr.packed_entries(int(blocks), src_scale, geom=geom)
    if got is None or env == "1":
        return got
    return got if rule(csr.n_cols, int(blocks), got[2], nat.PACKED_IDX_BITS) else None


# element types of the hop's table and output -> HGD_DT_* (hgd_spmm_dt)
_HOP_DTYPES = {torch.float32: nat.DT_F32, torch.bfloat16: nat.DT_BF16}


def _hop_names(fused16: bool) -> Tuple[str, str]:
    """Who rejects a call that reached :func:`spmm_csr`'s checks and what it calls its table:
    :func:`spmm_csr_fused_dt` and ``X16`` when the call came through that function."""
    return ("spmm_fused_dt", "X16") if fused16 else ("spmm", "X")


def spmm_csr(csr: CSR, X: torch.Tensor, val: Optional[torch.Tensor] = None,
             row_scale: Optional[torch.Tensor] = None, epilogue: int = nat.EPI_NONE,
             slope: float = 0.0, out: Optional[torch.Tensor] = None,
             row_begin: int = 0, row_end: Optional[int] = None,
             ex: Optional[nat.RowEpilogue] = None, blocks: Optional[int] = None,
             out_dtype: Optional[torch.dtype] = None, _fused16: bool = False,
             _out16: Optional[torch.Tensor] = None,
             src_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Y[r] = epi(row_scale[r] * Σ_e val[e] * X[col[e]])`` for r in [row_begin, row_end).

    ``src_scale`` (float32 ``[n_cols]``): the caller's statement that ``val`` is that scale over
    the source rows expanded per nonzero, ``val[e] = src_scale[col[e]]`` bit for bit. The fp32
    block-ordered hop then runs on packed entries without the weight stream when
    :func:`spmm_packed` says so (hgd_spmm_blocked_packed, the same Y bit for bit); every other
    hop reads ``val`` as without it, so ``src_scale`` without ``val`` on such a hop is an error.

    ``X`` is float32 or bfloat16; the result is ``out.dtype`` if ``out`` is given, else
    ``out_dtype``, else ``X.dtype``. Float32 in and out is hgd_spmm (and its masked / blocked /
    fused forms); a bfloat16 side is hgd_spmm_dt / hgd_spmm_masked_dt: the same fp32 sums over
    exactly widened elements, a bf16 result rounded to nearest even on the store. A bf16 hop has
    no fused row epilogue (``ex``) here: that is :func:`spmm_csr_fused_dt`, asked for by name.
    Source-blocked it is hgd_spmm_blocked_dt, whose bf16 result is still the fp32 result rounded
    once (the blocks' partials stay fp32, in a scratch).

    With ``ex`` (an ``hgd_row_epilogue``) the call is ``hgd_spmm_fused``: ``ex.act``/``ex.slope``
    replace ``epilogue``/``slope`` and the LayerNorm / residual epilogue runs in the store.
    ``blocks``: None = :func:`spmm_blocks` decides whether the hop runs source-blocked
    (hgd_spmm_blocked) and, for an fp32 hop over a structure with split rows,
    :func:`spmm_blocks_split` whether it runs as hgd_spmm_blocked_split; 0 = never (e.g. into
    uncached exchange memory, which the blocked hop would read back P−1 times).

    A hop over all rows that is not source-blocked walks the structure's row order when
    :func:`spmm_row_order` says so for its form — plain, masked, fused, 16-bit or any of them
    together (hgd_spmm_ordered and the ordered twins of the other entry points): the same bits in
    every output. An edge-dropped view takes the order from its parent (:meth:`CSR.order_source`)
    and adds one byte gather of its mask (:meth:`CSR.ordered_mask`).

    ``_fused16`` / ``_out16`` are :func:`spmm_csr_fused_dt`'s, which runs this body after its
    own checks: the one 16-bit hop that takes ``ex``, and its bf16 copy of the result. A
    rejection then speaks in that function's words (:func:`_hop_names`)."""
    if X.dim() != 2:
        raise ValueError("%s: %s must be 2-D, got %s" % (*_hop_names(_fused16), tuple(X.shape)))
    if X.dtype not in _HOP_DTYPES:
        raise TypeError(f"spmm: X must be float32 or bfloat16, got {X.dtype}")
    y_dtype = out.dtype if out is not None else (out_dtype or X.dtype)
    if y_dtype not in _HOP_DTYPES:
        raise TypeError(f"spmm: the output must be float32 or bfloat16, got {y_dtype}")
    dt = X.dtype != torch.float32 or y_dtype != torch.float32  # a 16-bit side: the _dt entries
    if dt and ex is not None and not _fused16:
        raise TypeError("spmm: the fused row epilogue (ex=) is float32-only; a bfloat16 "
                        f"table or output cannot take it (X {X.dtype}, output {y_dtype})")
    if X.device.type != "cuda":
        raise RuntimeError("%s: %s must be a device (cuda/hip) tensor; there is no CPU path"
                           % _hop_names(_fused16))
    if X.shape[0] != csr.n_cols:
        raise ValueError("%s: %s has %d rows, structure expects %d"
                         % (*_hop_names(_fused16), X.shape[0], csr.n_cols))
    if X.stride(1) != 1:
        X = X.contiguous()
    d = X.shape[1]
    if out is None:
        out = torch.empty((csr.n_rows, d), dtype=y_dtype, device=X.device)
    if row_end is None:
        row_end = csr.n_rows
    if d == 0 or row_end <= row_begin:
        return out
    if val is not None and val.numel() != csr.nnz:
        raise ValueError(f"{_hop_names(_fused16)[0]}: val size mismatch")
    if row_scale is not None and row_scale.numel() != csr.n_rows:
        raise ValueError(f"{_hop_names(_fused16)[0]}: row_scale size mismatch")
    lib = nat.load()
    plan_ptr = ctypes.byref(csr.plan)
    # the plan is immutable once built: its workspace size per width is asked for once
    wsb = csr._ws_bytes.get(d)
    if wsb is None:
        wsb = csr._ws_bytes[d] = lib.hgd_spmm_workspace_size(plan_ptr, d)
    ws = _ws(wsb, X.device) if wsb else None
    timer = profiling.active()
    if timer is not None:
        t0 = timer.begin()
    mask = getattr(csr, "mask", None)
    split_blocks = 0  # the blocks of a structure with split rows (hgd_spmm_blocked_split)
    if mask is not None or ex is not None or blocks == 0:
        blocks = 0
    else:
        blocks = spmm_blocks(csr, d, X.dtype)
        if not blocks and not dt and csr.n_heavy:  # spmm_blocks' 0 is for the split rows
            split_blocks = spmm_blocks_split(csr, d, X.dtype)
    # the arguments the entry points share, evaluated once: the structure (a masked one adds its
    # mask and keep rate), row scale and row range, the table and the output, workspace and stream.
    # (Plain locals passed positionally: packing them into tuples and unpacking those into the
    # calls measured 0.3 µs per call slower on this path, which runs on every eager step.)
    rp, cp, vp = csr.rowptr.data_ptr(), csr.col.data_ptr() if csr.nnz else None, nat.ptr(val)
    if mask is not None:
        mp, keep = mask.data_ptr() if csr.nnz else None, float(csr.keep)
    sp, n, m, rb, re_ = nat.ptr(row_scale), csr.n_rows, csr.n_cols, int(row_begin), int(row_end)
    xp, ldx, yp, ldy = X.data_ptr(), X.stride(0), out.data_ptr(), out.stride(0)
    wp, st = nat.ptr(ws), _stream(X.device)
    # a hop over the whole row range that is not source-blocked may walk its rows in an order of
    # its own (min column, or greedy shared-column: kind below) — the plain fp32 hop by its size
    # rule, a masked, fused or 16-bit one by the rule of its form
    if dt or mask is not None or ex is not None:
        ordered = (not blocks and rb == 0 and re_ == n
                   and spmm_row_order(csr, d, X.dtype, y_dtype, ex is not None, mask is not None))
    else:
        ordered = not blocks and rb == 0 and re_ == n and spmm_row_order(csr, d)
    # and the fp32 source-blocked hop over the whole row range each block's rows in its own
    blk_ordered = (not dt and bool(blocks) and rb == 0 and re_ == n
                   and spmm_block_order(csr, d, blocks))
    # which order such a hop walks: min column, or the greedy shared-column order
    kind = spmm_order_kind(csr, d, blocks) if ordered or blk_ordered else nat.ORDER_NONE
    # (None: the min-column order; the geometry is read once per hop, the orders' cache key)
    if kind != nat.ORDER_GREEDY:
        geom = None
    elif ordered and (dt or ex is not None):
        # of the form that runs: its lanes, its passes, its gathered piece (a mask changes none)
        geom = order_geometry(d, False, X.dtype, y_dtype, ex is not None)
    else:
        geom = order_geometry(d, bool(blocks))
    # ... on packed entries when the weights are a source-row scale with few distinct values
    packed = spmm_packed(csr, blocks, src_scale, geom) if blk_ordered else None
    if src_scale is not None:
        if src_scale.dtype != torch.float32 or src_scale.numel() != m:
            raise ValueError(f"{_hop_names(_fused16)[0]}: src_scale must be float32 [n_cols]")
        if val is None and packed is None:
            raise ValueError(f"{_hop_names(_fused16)[0]}: src_scale without val on a hop that "
                             "does not run on packed entries (pass the expanded val beside it)")
    if packed is not None:
        start, _, _, out_row = csr._blocks_of(blocks, geom)
        ent, wdict, n_dict = packed
        nat.check(lib.hgd_spmm_blocked_packed(
            start.data_ptr(), ent.data_ptr(), wdict.data_ptr(), n_dict, nat.PACKED_IDX_BITS,
            nat.ptr(csr.blocked_ordered_scale(blocks, row_scale, geom)), out_row.data_ptr(), n,
            m, xp, ldx, yp, ldy, d, int(epilogue), float(slope), blocks, st),
            "hgd_spmm_blocked_packed")
    elif ordered:
        # the order and the ordered weights / scales are the structure's: an edge-dropped view
        # takes them from its parent (built once, not once per step) and brings its mask alone
        src = csr.order_source()
        order, rowptr_o, col_o, _ = src._rows_of(geom)
        rp, cp, op = rowptr_o.data_ptr(), col_o.data_ptr(), order.data_ptr()
        vp, sp = nat.ptr(src.ordered_values(val, geom)), nat.ptr(src.ordered_scale(row_scale, geom))
        if mask is not None:
            mp = csr.ordered_mask(geom).data_ptr()
        if _fused16:
            y16p, ld16 = nat.ptr(_out16), 0 if _out16 is None else _out16.stride(0)
            if mask is not None:
                nat.check(lib.hgd_spmm_masked_fused_ordered_dt(
                    rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, nat.DT_BF16, ldx, yp, ldy, d,
                    ctypes.byref(ex), y16p, ld16, plan_ptr, wp, wsb, op, st),
                    "hgd_spmm_masked_fused_ordered_dt")
            else:
                nat.check(lib.hgd_spmm_fused_ordered_dt(
                    rp, cp, vp, sp, n, m, rb, re_, xp, nat.DT_BF16, ldx, yp, ldy, d,
                    ctypes.byref(ex), y16p, ld16, plan_ptr, wp, wsb, op, st),
                    "hgd_spmm_fused_ordered_dt")
        elif dt and mask is not None:
            nat.check(lib.hgd_spmm_masked_ordered_dt(
                rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, _HOP_DTYPES[X.dtype], ldx, yp,
                _HOP_DTYPES[y_dtype], ldy, d, int(epilogue), float(slope), plan_ptr, wp, wsb, op,
                st), "hgd_spmm_masked_ordered_dt")
        elif dt:
            nat.check(lib.hgd_spmm_ordered_dt(
                rp, cp, vp, sp, n, m, rb, re_, xp, _HOP_DTYPES[X.dtype], ldx, yp,
                _HOP_DTYPES[y_dtype], ldy, d, int(epilogue), float(slope), plan_ptr, wp, wsb, op,
                st), "hgd_spmm_ordered_dt")
        elif mask is not None and ex is not None:
            nat.check(lib.hgd_spmm_masked_fused_ordered(
                rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, ctypes.byref(ex),
                plan_ptr, wp, wsb, op, st), "hgd_spmm_masked_fused_ordered")
        elif mask is not None:
            nat.check(lib.hgd_spmm_masked_ordered(
                rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, int(epilogue),
                float(slope), plan_ptr, wp, wsb, op, st), "hgd_spmm_masked_ordered")
        elif ex is not None:
            nat.check(lib.hgd_spmm_fused_ordered(
                rp, cp, vp, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, ctypes.byref(ex), plan_ptr,
                wp, wsb, op, st), "hgd_spmm_fused_ordered")
        else:
            nat.check(lib.hgd_spmm_ordered(
                rp, cp, vp, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, int(epilogue), float(slope),
                plan_ptr, wp, wsb, op, st), "hgd_spmm_ordered")
    elif _fused16:  # (ex: never blocked)
        y16p, ld16 = nat.ptr(_out16), 0 if _out16 is None else _out16.stride(0)
        if mask is not None:
            nat.check(lib.hgd_spmm_masked_fused_dt(
                rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, nat.DT_BF16, ldx, yp, ldy, d,
                ctypes.byref(ex), y16p, ld16, plan_ptr, wp, wsb, st), "hgd_spmm_masked_fused_dt")
        else:
            nat.check(lib.hgd_spmm_fused_dt(
                rp, cp, vp, sp, n, m, rb, re_, xp, nat.DT_BF16, ldx, yp, ldy, d,
                ctypes.byref(ex), y16p, ld16, plan_ptr, wp, wsb, st), "hgd_spmm_fused_dt")
    elif dt and mask is not None:
        nat.check(lib.hgd_spmm_masked_dt(
            rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, _HOP_DTYPES[X.dtype], ldx, yp,
            _HOP_DTYPES[y_dtype], ldy, d, int(epilogue), float(slope), plan_ptr, wp, wsb, st),
            "hgd_spmm_masked_dt")
    elif dt and blocks:
        start, bcol, _ = csr.col_blocks(blocks)
        bval = csr.blocked_values(blocks, val)
        # a bf16 output keeps its fp32 running partials in a scratch (an fp32 one in itself)
        pb = lib.hgd_spmm_blocked_dt_workspace_size(n, d, _HOP_DTYPES[y_dtype], blocks)
        part = _ws(pb, X.device) if pb else None
        nat.check(lib.hgd_spmm_blocked_dt(
            start.data_ptr(), bcol.data_ptr(), nat.ptr(bval), sp, n, m, rb, re_, xp,
            _HOP_DTYPES[X.dtype], ldx, yp, _HOP_DTYPES[y_dtype], ldy, d, int(epilogue),
            float(slope), blocks, nat.ptr(part), pb, st), "hgd_spmm_blocked_dt")
    elif dt:
        nat.check(lib.hgd_spmm_dt(
            rp, cp, vp, sp, n, m, rb, re_, xp, _HOP_DTYPES[X.dtype], ldx, yp,
            _HOP_DTYPES[y_dtype], ldy, d, int(epilogue), float(slope), plan_ptr, wp, wsb, st),
            "hgd_spmm_dt")
    elif mask is not None and ex is not None:
        nat.check(lib.hgd_spmm_masked_fused(
            rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, ctypes.byref(ex),
            plan_ptr, wp, wsb, st), "hgd_spmm_masked_fused")
    elif mask is not None:
        nat.check(lib.hgd_spmm_masked(
            rp, cp, vp, mp, keep, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, int(epilogue),
            float(slope), plan_ptr, wp, wsb, st), "hgd_spmm_masked")
    elif blk_ordered:  # (blocks: no mask, no fused epilogue)
        start, bcol, _, out_row = csr._blocks_of(blocks, geom)
        nat.check(lib.hgd_spmm_blocked_ordered(
            start.data_ptr(), bcol.data_ptr(),
            nat.ptr(csr.blocked_ordered_values(blocks, val, geom)),
            nat.ptr(csr.blocked_ordered_scale(blocks, row_scale, geom)), out_row.data_ptr(), n,
            m, xp, ldx, yp, ldy, d, int(epilogue), float(slope), blocks, st),
            "hgd_spmm_blocked_ordered")
    elif split_blocks:  # (fp32, no mask, no fused epilogue)
        start, bcol, _ = csr.col_blocks(split_blocks)
        plans = csr.col_block_plans(split_blocks)
        pb = csr._blk_ws_bytes.get((split_blocks, d))
        if pb is None:
            pb = csr._blk_ws_bytes[(split_blocks, d)] = lib.hgd_spmm_blocked_split_workspace_size(
                plans, split_blocks, d)
        part = _ws(pb, X.device) if pb else None
        nat.check(lib.hgd_spmm_blocked_split(
            start.data_ptr(), bcol.data_ptr(), nat.ptr(csr.blocked_values(split_blocks, val)), sp,
            n, m, rb, re_, xp, ldx, yp, ldy, d, int(epilogue), float(slope), split_blocks, plans,
            nat.ptr(part), pb, st), "hgd_spmm_blocked_split")
    elif ex is None and blocks:
        start, bcol, _ = csr.col_blocks(blocks)
        bval = csr.blocked_values(blocks, val)
        nat.check(lib.hgd_spmm_blocked(
            start.data_ptr(), bcol.data_ptr(), nat.ptr(bval), sp, n, m, rb, re_, xp, ldx, yp,
            ldy, d, int(epilogue), float(slope), blocks, st), "hgd_spmm_blocked")
    elif ex is None:
        nat.check(lib.hgd_spmm(
            rp, cp, vp, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, int(epilogue), float(slope),
            plan_ptr, wp, wsb, st), "hgd_spmm")
    else:
        nat.check(lib.hgd_spmm_fused(
            rp, cp, vp, sp, n, m, rb, re_, xp, ldx, yp, ldy, d, ctypes.byref(ex), plan_ptr, wp,
            wsb, st), "hgd_spmm_fused")
    if timer is not None:
        full = rb == 0 and re_ == csr.n_rows

        def nbytes(csr=csr, rb=rb, re_=re_, full=full, d=d, hv=val is not None,
                   hs=row_scale is not None, blocks=blocks or split_blocks,
                   xb=X.element_size(), yb=out.element_size(), ordered=ordered,
                   blk_ordered=blk_ordered, split=bool(split_blocks),
                   packed=packed is not None):
            nnz = csr.nnz if full else int(csr.rowptr[re_].item() - csr.rowptr[rb].item())
            # (the chunks of every split row: a row range runs those of its own rows only)
            chunks = sum(int(p.n_chunks) for p in csr.col_block_plans(blocks)) if split else 0
            return (profiling.hop_bytes(nnz, re_ - rb, d, x_bytes=xb, y_bytes=yb),
                    profiling.impl_bytes(nnz, re_ - rb, d, hv, hs, blocks, x_bytes=xb,
                                         y_bytes=yb, ordered=ordered,
                                         block_ordered=blk_ordered, split_chunks=chunks,
                                         packed=packed))

        timer.end(t0, nbytes)
    return out


def spmm_csr_fused_dt(csr: CSR, X16: torch.Tensor, ex: nat.RowEpilogue,
                      val: Optional[torch.Tensor] = None,
                      row_scale: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None,
                      row_begin: int = 0, row_end: Optional[int] = None) -> torch.Tensor:
    """The hop with the fused row epilogue ``ex`` gathering from the bfloat16 table ``X16``
    (hgd_spmm_fused_dt; hgd_spmm_masked_fused_dt over an edge-dropped view): ``Y[r] =
    ex(row_scale[r] * Σ_e val[e] * X16[col[e]])`` for r in [row_begin, row_end), a float32
    result. Everything ``ex`` points to is float32, as for ``spmm_csr(..., ex=)``; the sums are
    fp32 over exactly widened elements.

    ``out16`` (bfloat16 [n_rows, d]) is filled with the rows of Y rounded to nearest even, from
    the registers Y was stored from: the table a following hop gathers. Never source-blocked,
    like the fp32 fused hop; over all rows it walks the structure's row order where
    :func:`spmm_row_order` turns it on for this form (hgd_spmm_fused_ordered_dt /
    hgd_spmm_masked_fused_ordered_dt: the same bits, ``out`` and ``out16`` rows included)."""
    if X16.dtype != torch.bfloat16:
        raise TypeError(f"spmm_fused_dt: X16 must be bfloat16, got {X16.dtype}")
    if out is not None and out.dtype != torch.float32:
        raise TypeError(f"spmm_fused_dt: the output must be float32, got {out.dtype}")
    if out16 is not None and out16.dtype != torch.bfloat16:
        raise TypeError(f"spmm_fused_dt: out16 must be bfloat16, got {out16.dtype}")
    if ex is None:
        raise ValueError("spmm_fused_dt: needs a row epilogue (ex)")
    if X16.dim() == 2:  # (any other is the shared checks' to reject)
        shape = (csr.n_rows, X16.shape[1])
        for name, t in (("out", out), ("out16", out16)):
            if t is not None and (tuple(t.shape) != shape or t.stride(1) != 1
                                  or t.device != X16.device):
                raise ValueError(f"spmm_fused_dt: {name} must be a [{shape[0]}, {shape[1]}] "
                                 f"matrix with unit column stride on {X16.device}")
    # the shared checks, the plan's workspace, the launch and the timer's record are spmm_csr's
    return spmm_csr(csr, X16, val, row_scale, nat.EPI_NONE, 0.0, out, row_begin, row_end, ex, 0,
                    torch.float32, True, out16)


class Incidence:
    """Sparse ``A [n_rows, n_cols]`` as CSR + CSC on the device (see module docstring)."""

    def __init__(self, csr: CSR, csc: CSR, val: Optional[torch.Tensor],
                 val_t: Optional[torch.Tensor]):
        self.csr = csr
        self.csc = csc
        self.val = val          # per-nonzero weights in CSR order (None = binary)
        self.val_t = val_t      # the same weights in CSC order
        self.n_rows = csr.n_rows
        self.n_cols = csr.n_cols
        self.nnz = csr.nnz
        self.device = csr.device
        self._scales: Dict[Tuple[str, str], torch.Tensor] = {}
        self._edge_vals: Dict[Tuple[str, str, str], Optional[torch.Tensor]] = {}
        self.perm_t: Optional[torch.Tensor] = None  # CSC position → CSR position
        self.coo_sorted = False  # True when built from a row-sorted COO (COO order = CSR order)

    @property
    def shape(self):
        return (self.n_rows, self.n_cols)

    def __deepcopy__(self, memo):
        return self  # immutable once built (scale / edge-value caches are derived data)

    # -- construction ------------------------------------------------------------------
    @classmethod
    def from_coo(cls, indices: torch.Tensor, values: Optional[torch.Tensor], shape,
                 device=None, validate: bool = True, rows_sorted: Optional[bool] = None,
                 split_threshold: Optional[int] = None,
                 split_chunk: Optional[int] = None) -> "Incidence":
        """Builds from COO ``indices`` int64 [2, nnz] (+ fp32 ``values`` or None = ones).

        ``split_threshold`` / ``split_chunk`` default to :func:`auto_split` per orientation.

        Entries keep their order within a row (duplicates stay separate nonzeros, which is the
        same linear map as torch's coalesced sum). Raises ValueError on out-of-range indices.
        """
        n_rows, n_cols = int(shape[0]), int(shape[1])
        if n_rows >= 2 ** 31 or n_cols >= 2 ** 31:
            raise ValueError("Incidence: dimensions must be < 2^31")
        device = torch.device(device) if device is not None else indices.device
        if device.type != "cuda":
            raise RuntimeError("Incidence: needs a device (cuda/hip) target; there is no CPU path")
        lib = nat.load()
        st = _stream(device)
        indices = indices.to(device=device, dtype=torch.int64)
        nnz = int(indices.shape[1])
        if values is not None:
            values = values.to(device=device, dtype=torch.float32).contiguous()
            if values.numel() != nnz:
                raise ValueError("Incidence: values/indices size mismatch")
        rows64 = indices[0].contiguous()
        cols64 = indices[1].contiguous()
        rows = torch.empty(nnz, dtype=torch.int32, device=device)
        cols = torch.empty(nnz, dtype=torch.int32, device=device)
        flags = torch.zeros(3, dtype=torch.int64, device=device)
        if nnz:
            nat.check(lib.hgd_index_narrow(rows64.data_ptr(), nnz, n_rows, rows.data_ptr(),
                                           flags[0:1].data_ptr(), st), "hgd_index_narrow(rows)")
            nat.check(lib.hgd_index_narrow(cols64.data_ptr(), nnz, n_cols, cols.data_ptr(),
                                           flags[1:2].data_ptr(), st), "hgd_index_narrow(cols)")
            if rows_sorted is None:
                nat.check(lib.hgd_check_sorted(rows.data_ptr(), nnz, n_rows,
                                               flags[2:3].data_ptr(), st), "hgd_check_sorted")
        if validate or rows_sorted is None:
            f = flags.tolist()
            if f[0] or f[1]:
                raise ValueError(f"Incidence: {f[0]} row / {f[1]} col indices out of range "
                                 f"for shape {(n_rows, n_cols)}")
            if rows_sorted is None:
                rows_sorted = f[2] == 0
        if nnz and not rows_sorted:
            perm = torch.empty(nnz, dtype=torch.int32, device=device)
            rows_s = torch.empty_like(rows)
            ws = _ws(lib.hgd_sort_perm_workspace_size(nnz), device)
            nat.check(lib.hgd_sort_perm(rows.data_ptr(), nnz, n_rows, rows_s.data_ptr(),
                                        perm.data_ptr(), ws.data_ptr(), ws.numel(), st),
                      "hgd_sort_perm(rows)")
            rows = rows_s
            cols = _gather32(cols, perm)
            if values is not None:
                values = _gather32(values, perm)
        inc = cls._from_sorted(rows, cols, values, n_rows, n_cols, split_threshold, split_chunk)
        inc.coo_sorted = bool(rows_sorted) or nnz == 0
        return inc

    @classmethod
    def _from_sorted(cls, rows: torch.Tensor, cols: torch.Tensor, values: Optional[torch.Tensor],
                     n_rows: int, n_cols: int, split_threshold: Optional[int] = None,
                     split_chunk: Optional[int] = None) -> "Incidence":
        device = rows.device
        lib = nat.load()
        st = _stream(device)
        nnz = int(rows.numel())
        rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=device)
        nat.check(lib.hgd_rowptr_from_sorted(rows.data_ptr() if nnz else None, nnz, n_rows,
                                             rowptr.data_ptr(), st), "hgd_rowptr_from_sorted")
        # CSC: stable sort of the column ids keeps rows ascending inside each column.
        colptr = torch.empty(n_cols + 1, dtype=torch.int64, device=device)
        csc_col = torch.empty(nnz, dtype=torch.int32, device=device)
        val_t = None
        if nnz:
            keys = torch.empty(nnz, dtype=torch.int32, device=device)
            perm = torch.empty(nnz, dtype=torch.int32, device=device)
            ws = _ws(lib.hgd_sort_perm_workspace_size(nnz), device)
            nat.check(lib.hgd_sort_perm(cols.data_ptr(), nnz, n_cols, keys.data_ptr(),
                                        perm.data_ptr(), ws.data_ptr(), ws.numel(), st),
                      "hgd_sort_perm(cols)")
            del ws
            nat.check(lib.hgd_rowptr_from_sorted(keys.data_ptr(), nnz, n_cols,
                                                 colptr.data_ptr(), st),
                      "hgd_rowptr_from_sorted(csc)")
            del keys
            csc_col = _gather32(rows, perm)
            if values is not None:
                val_t = _gather32(values, perm)
        else:
            colptr.zero_()
            perm = torch.empty(0, dtype=torch.int32, device=device)

        def split(n):
            if split_threshold is None:
                return auto_split(n, nnz)
            return split_threshold, split_chunk or DEFAULT_SPLIT_CHUNK

        csr = CSR(rowptr, cols, n_rows, n_cols, *split(n_rows))
        csc = CSR(colptr, csc_col, n_cols, n_rows, *split(n_cols))
        csc.cols_ascending = True
        c1, c2 = csr.plan_count_async(), csc.plan_count_async()
        if c1 is not None:
            csr._build_plan(*c1.tolist())
        if c2 is not None:
            csc._build_plan(*c2.tolist())
        csr.configure_kernel()
        csc.configure_kernel()
        inc = cls(csr, csc, values, val_t)
        inc.perm_t = perm  # CSC position → CSR position (sort-free drop-edge rebuilds)
        return inc

    def persist(self) -> "Incidence":
        """Says that this structure outlives the steps that hop over it (a dataset's graph, held
        for a whole run): its hops may then walk the greedy shared-column order, built on the
        host once with a stream synchronisation (:func:`spmm_order_kind`). Never say it of a
        structure made per step. Returns ``self``."""
        self.csr.persistent = self.csc.persistent = True
        return self

    def drop(self, mask: torch.Tensor, keep: float, kept: Optional[int] = None,
             capacity: bool = False) -> "Incidence":
        """The incidence of SpAdjDropEdge's output (HCCF.py:217-226) built from this one without
        any sort: ``mask`` (uint8/bool, CSR order) keeps nonzeros in order and values are divided
        by ``keep``; the CSC comes from compacting this CSC through ``perm_t``
        (hgd_dropedge_structure). One device→host read (the kept count) unless the caller passes
        ``kept`` (e.g. counted with a host-drawn mask) or asks for ``capacity``: then the kept
        count stays on the device (the row pointers end at it), the arrays keep the parent's
        length with a zeroed tail (hgd_dropedge_fill_tail), and rows longer than the split
        threshold are walked by one lane group (no split plan: it would need the count) — no
        host read, so a training step can be captured in a HIP graph."""
        lib = nat.load()
        dev = self.device
        st = _stream(dev)
        nnz, R, C = self.nnz, self.n_rows, self.n_cols
        m = mask.to(device=dev, dtype=torch.uint8).contiguous()
        if m.numel() != nnz:
            raise ValueError("Incidence.drop: mask size mismatch")
        rowptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
        colptr = torch.empty(C + 1, dtype=torch.int64, device=dev)
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        row_t = torch.empty(nnz, dtype=torch.int32, device=dev)
        weighted = self.val is not None
        val = torch.empty(nnz, dtype=torch.float32, device=dev) if weighted else None
        val_t = torch.empty(nnz, dtype=torch.float32, device=dev) if weighted else None
        ws = _ws(lib.hgd_dropedge_structure_workspace_size(nnz), dev)
        nat.check(lib.hgd_dropedge_structure(
            self.csr.rowptr.data_ptr(), nat.ptr(self.csr.col) if nnz else None, nat.ptr(self.val),
            self.csc.rowptr.data_ptr(), nat.ptr(self.csc.col) if nnz else None,
            nat.ptr(self.val_t), nat.ptr(self.perm_t) if nnz else None, R, C, nnz,
            m.data_ptr() if nnz else None, float(keep), rowptr.data_ptr(),
            col.data_ptr() if nnz else None, nat.ptr(val), colptr.data_ptr(),
            row_t.data_ptr() if nnz else None, nat.ptr(val_t), ws.data_ptr(), ws.numel(), st),
            "hgd_dropedge_structure")
        if capacity:
            if nnz:
                nat.check(lib.hgd_dropedge_fill_tail(
                    rowptr.data_ptr() + 8 * R, nnz, col.data_ptr(), nat.ptr(val),
                    row_t.data_ptr(), nat.ptr(val_t), st), "hgd_dropedge_fill_tail")
            csr = CSR(rowptr, col, R, C, 0, self.csr.split_chunk)
            csc = CSR(colptr, row_t, C, R, 0, self.csc.split_chunk)
            for child, parent in ((csr, self.csr), (csc, self.csc)):
                child.plan.flags = parent.plan.flags if parent.n_heavy == 0 else 0
            out = Incidence(csr, csc, val, val_t)
            out.perm_t = None
            return out
        if kept is None:
            kept = int(rowptr[R].item()) if R else 0
        col, row_t = col[:kept], row_t[:kept]
        if weighted:
            val, val_t = val[:kept], val_t[:kept]
        csr = CSR(rowptr, col, R, C, self.csr.split_threshold, self.csr.split_chunk)
        csc = CSR(colptr, row_t, C, R, self.csc.split_threshold, self.csc.split_chunk)
        # degrees only shrink: a parent without split rows has none after dropping (no count)
        for child, parent in ((csr, self.csr), (csc, self.csc)):
            if parent.n_heavy:
                cnt = child.plan_count_async()
                if cnt is not None:
                    child._build_plan(*cnt.tolist())
            child.plan.flags = parent.plan.flags if child.n_heavy == 0 else 0
        out = Incidence(csr, csc, val, val_t)
        out.perm_t = None  # a dropped structure is not dropped again (the reference drops the base)
        return out

    def masked(self, mask: torch.Tensor, keep: float,
               mask_t: Optional[torch.Tensor] = None) -> "MaskedIncidence":
        """SpAdjDropEdge's output (HCCF.py:217-226) as a VIEW of this incidence: no compaction
        at all. The hops run over this structure and skip the dropped edges
        (hgd_spmm_masked: weight val[e] / keep, kept edges in edge order — the sums of the
        compacted matrix of :meth:`drop`, bitwise when no row is split). The CSC-order mask is
        one byte gather through ``perm_t``; nothing is read back to the host, so a step using
        it can be captured in a HIP graph. For the plain hops (GCNLayer, HGCNConv without
        degree scales); degree scales of the dropped matrix need :meth:`drop`. ``mask_t``: the
        same mask already in CSC order (hgd_bernoulli_mask_dev_pair draws both)."""
        if self.perm_t is None:
            raise RuntimeError("Incidence.masked: needs the CSC→CSR permutation (a structure "
                               "built from a COO)")
        dev = self.device
        m = mask.to(device=dev, dtype=torch.uint8).contiguous()
        if m.numel() != self.nnz:
            raise ValueError("Incidence.masked: mask size mismatch")
        if not keep > 0.0:
            raise ValueError("Incidence.masked: keep must be > 0")
        if mask_t is not None:
            m_t = mask_t.to(device=dev, dtype=torch.uint8).contiguous()
            if m_t.numel() != self.nnz:
                raise ValueError("Incidence.masked: mask_t size mismatch")
        else:
            m_t = torch.empty_like(m)
            if self.nnz:
                nat.check(nat.load().hgd_gather_u8(m.data_ptr(), self.perm_t.data_ptr(),
                                                   self.nnz, m_t.data_ptr(), _stream(dev)),
                          "hgd_gather_u8")
        csr = copy.copy(self.csr)
        csc = copy.copy(self.csc)
        csr.mask, csr.keep = m, float(keep)
        csc.mask, csc.keep = m_t, float(keep)
        # a view is made on every step: the row orders and what is gathered through them are the
        # parent's (CSR.order_source), the mask in an order's entry order is the view's own
        for view, parent in ((csr, self.csr), (csc, self.csc)):
            view._order_parent = parent.order_source()
            view._mask_ord = {}
        out = MaskedIncidence(csr, csc, self.val, self.val_t)
        out.parent = self
        return out

    @classmethod
    def from_dense(cls, A: torch.Tensor, device=None, **kw) -> "Incidence":
        """The nonzero pattern and values of a dense matrix (``torch.nonzero(A)`` order), e.g.
        DHCF's dense interaction matrix fed to HGCNConv (DHCF.py:140, :131-133)."""
        device = torch.device(device) if device is not None else (
            A.device if A.device.type == "cuda" else torch.device("cuda"))
        A = A.to(device=device, dtype=torch.float32)
        rowptr, cols, vals = dense_threshold(A, 0.0, nonzero=True, values=True)
        rows = expand_rows(rowptr, cols.numel())
        inc = cls._from_sorted(rows, cols, vals, A.shape[0], A.shape[1], **kw)
        inc.coo_sorted = True
        return inc

    @classmethod
    def from_torch_sparse(cls, adj: torch.Tensor, device=None, **kw) -> "Incidence":
        """From a torch sparse COO tensor as built by ``convert_sparse_mat_to_tensor``."""
        if adj.layout != torch.sparse_coo:
            raise TypeError("Incidence.from_torch_sparse expects a sparse COO tensor")
        if device is None:
            device = adj.device if adj.device.type == "cuda" else torch.device("cuda")
        return cls.from_coo(adj._indices(), adj._values(), adj.shape, device=device, **kw)

    @classmethod
    def from_scipy(cls, mat, device="cuda", binary: bool = False, **kw) -> "Incidence":
        """From a scipy sparse matrix (row-major COO order of ``tocoo()``, like the reference)."""
        coo = mat.tocoo()
        idx = torch.stack([torch.from_numpy(coo.row.astype("int64")),
                           torch.from_numpy(coo.col.astype("int64"))])
        vals = None if binary else torch.from_numpy(coo.data.astype("float32"))
        return cls.from_coo(idx, vals, coo.shape, device=device, **kw)

    @classmethod
    def from_index_lists(cls, vertex: torch.Tensor, edges: torch.Tensor, n_vertices: int,
                         n_edges: Optional[int] = None, device=None, **kw) -> "Incidence":
        """Binary incidence B[vertex[k], edges[k]] (ED-HNN's V/E lists, EquivSetConv2.py:85-93).

        ``n_edges`` defaults to max(edges)+1, the row count torch_scatter gives the edge means.
        """
        device = torch.device(device) if device is not None else vertex.device
        if device.type != "cuda":
            device = torch.device("cuda")
        if n_edges is None:
            n_edges = int(edges.max().item()) + 1 if edges.numel() else 0
        idx = torch.stack([vertex.to(device=device, dtype=torch.int64),
                           edges.to(device=device, dtype=torch.int64)])
        return cls.from_coo(idx, None, (int(n_vertices), int(n_edges)), device=device, **kw)

    # -- derived per-row / per-nonzero quantities --------------------------------------
    def scale(self, side: str, kind: Optional[str]) -> Optional[torch.Tensor]:
        """Degree scale over rows ('row') or columns ('col') of A.

        kind: None → no scale; 'mean' → 1/deg (torch_scatter mean; 0 for empty);
        'sym' → deg^-1/2 (data/graph.py:15-16, inf→0); 'wmean'/'wsym' use the weighted
        degree Σ val (normalize_graph_mat's rowsum of a weighted matrix).
        """
        if kind is None:
            return None
        key = (side, kind)
        s = self._scales.get(key)
        if s is not None:
            return s
        o = self.csr if side == "row" else self.csc
        weighted = kind.startswith("w")
        power = {"mean": -1.0, "sym": -0.5}[kind[1:] if weighted else kind]
        w = None
        if weighted:
            w = self.val if side == "row" else self.val_t
        s = torch.empty(o.n_rows, dtype=torch.float32, device=self.device)
        nat.check(nat.load().hgd_degree_scale(o.rowptr.data_ptr(), nat.ptr(w), o.n_rows, power,
                                              s.data_ptr(), _stream(self.device)),
                  "hgd_degree_scale")
        self._scales[key] = s
        return s

    def edge_values(self, orient: str, src_kind: Optional[str]) -> Optional[torch.Tensor]:
        """Per-nonzero weights for a hop over ``orient`` ('csr' or 'csc') with the SOURCE-side
        diagonal folded in: w[e] = a[e] * S[src(e)], S = scale over the gathered side."""
        key = (orient, src_kind or "")
        if key in self._edge_vals:
            return self._edge_vals[key]
        o = self.csr if orient == "csr" else self.csc
        base = self.val if orient == "csr" else self.val_t
        src_side = "col" if orient == "csr" else "row"
        s = self.scale(src_side, src_kind)
        if s is None:
            out = base
        else:
            out = torch.empty(o.nnz, dtype=torch.float32, device=self.device)
            nat.check(nat.load().hgd_edge_values(
                nat.ptr(base), None, s.data_ptr(), o.col.data_ptr() if o.nnz else None, o.nnz,
                out.data_ptr(), _stream(self.device)), "hgd_edge_values")
        self._edge_vals[key] = out
        return out

    def edge_src_scale(self, orient: str, src_kind: Optional[str]) -> Optional[torch.Tensor]:
        """The scale over the gathered side that :meth:`edge_values` of the same arguments is
        the plain expansion of (``w[e] = S[src(e)]``), for ``spmm_csr(..., src_scale=)``; ``None``
        when the matrix has values of its own folded in, or no source scale."""
        base = self.val if orient == "csr" else self.val_t
        if base is not None:
            return None
        return self.scale("col" if orient == "csr" else "row", src_kind)

    def to_dense_cpu(self) -> torch.Tensor:
        """Debug helper: the matrix as a dense CPU tensor (test use)."""
        rp = self.csr.rowptr.cpu()
        rows = torch.repeat_interleave(torch.arange(self.n_rows), rp[1:] - rp[:-1])
        out = torch.zeros(self.n_rows, self.n_cols)
        v = self.val.cpu() if self.val is not None else torch.ones(self.nnz)
        out.index_put_((rows, self.csr.col.cpu().long()), v, accumulate=True)
        return out


class MaskedIncidence(Incidence):
    """An edge-dropped view of a parent incidence (:meth:`Incidence.masked`): both orientations
    share the parent's arrays and carry a keep-mask; hops skip the dropped edges. ``nnz`` is
    the parent's (the kept count stays on the device). Degree scales of the dropped matrix are
    not available on a view."""

    def scale(self, side: str, kind: Optional[str]) -> Optional[torch.Tensor]:
        if kind is None:
            return None
        raise NotImplementedError("MaskedIncidence: degree scales of an edge-dropped view; "
                                  "build the dropped structure with Incidence.drop")

    def materialize(self, capacity: bool = True) -> Incidence:
        """The compacted structure of the same drop (Incidence.drop)."""
        return self.parent.drop(self.csr.mask, self.csr.keep, capacity=capacity)


def drop_edges(indices: torch.Tensor, values: torch.Tensor, mask: torch.Tensor,
               keep_rate: float, count: Optional[int] = None):
    """Device compaction of SpAdjDropEdge (model/graph/HCCF.py:217-226): keeps the COO entries
    whose ``mask`` is set, in order, with ``values / keep_rate`` (IEEE fp32 division).
    Returns (indices int64 [2, kept], values fp32 [kept]). ``count`` (kept entries) avoids a
    device→host read when the caller already knows it (e.g. a host-drawn mask)."""
    device = values.device
    lib = nat.load()
    st = _stream(device)
    nnz = int(values.numel())
    indices = indices.to(device=device, dtype=torch.int64)
    rows = indices[0].contiguous()
    cols = indices[1].contiguous()
    m = mask.to(device=device, dtype=torch.uint8).contiguous()
    if m.numel() != nnz:
        raise ValueError("drop_edges: mask size mismatch")
    n_out = torch.empty(1, dtype=torch.int64, device=device)
    if count is None:
        count = int(m.sum().item()) if nnz else 0
    out_idx = torch.empty((2, count), dtype=torch.int64, device=device)
    out_val = torch.empty(count, dtype=torch.float32, device=device)
    if count == 0:  # nothing kept: nothing to write (the library takes no null output arrays)
        return out_idx, out_val
    ws = _ws(lib.hgd_dropedge_workspace_size(nnz), device)
    nat.check(lib.hgd_dropedge_compact(
        rows.data_ptr() if nnz else None, cols.data_ptr() if nnz else None,
        values.contiguous().data_ptr() if nnz else None, m.data_ptr() if nnz else None, nnz,
        float(keep_rate), out_idx[0].data_ptr() if count else None,
        out_idx[1].data_ptr() if count else None, out_val.data_ptr() if count else None,
        n_out.data_ptr(), ws.data_ptr(), ws.numel(), st), "hgd_dropedge_compact")
    return out_idx, out_val


def dense_threshold(H: torch.Tensor, thresh: float = 0.0, nonzero: bool = False,
                    values: bool = False):
    """``torch.nonzero(H > thresh)`` (or ``torch.nonzero(H)`` with ``nonzero=True``) of a dense
    2-D fp32 device matrix as CSR (rowptr int64 [n+1], cols int32 [nnz][, values fp32]) in
    row-major order (EquivSetGNN.generate_V_E, model/layers/layers2/EquivSetGNN2.py:105-133)."""
    if H.dim() != 2 or H.dtype != torch.float32:
        raise TypeError("dense_threshold: expects a 2-D float32 matrix")
    if H.stride(1) != 1:
        H = H.contiguous()
    device = H.device
    lib = nat.load()
    st = _stream(device)
    n, k = H.shape
    mode = 1 if nonzero else 0
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=device)
    ws = _ws(lib.hgd_dense_threshold_workspace_size(n), device)
    nat.check(lib.hgd_dense_threshold_rowptr(H.data_ptr(), n, k, H.stride(0), float(thresh),
                                             mode, rowptr.data_ptr(), ws.data_ptr(), ws.numel(),
                                             st), "hgd_dense_threshold_rowptr")
    nnz = int(rowptr[n].item())
    cols = torch.empty(nnz, dtype=torch.int32, device=device)
    vals = torch.empty(nnz, dtype=torch.float32, device=device) if values else None
    if nnz:
        nat.check(lib.hgd_dense_threshold_fill(H.data_ptr(), n, k, H.stride(0), float(thresh),
                                               mode, rowptr.data_ptr(), cols.data_ptr(),
                                               nat.ptr(vals), st), "hgd_dense_threshold_fill")
    if values:
        return rowptr, cols, vals
    return rowptr, cols


def expand_rows(rowptr: torch.Tensor, nnz: int) -> torch.Tensor:
    """Row id of every CSR nonzero (int32)."""
    n_rows = rowptr.numel() - 1
    out = torch.empty(nnz, dtype=torch.int32, device=rowptr.device)
    if nnz:
        nat.check(nat.load().hgd_expand_rows(rowptr.data_ptr(), n_rows, nnz, out.data_ptr(),
                                             _stream(rowptr.device)), "hgd_expand_rows")
    return out


def _gather32(src: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """``src[perm]`` over 4-byte elements: as long as ``perm``, which need not be ``src``'s
    length (a row scale gathered once per source block is n_blocks times as long)."""
    n = perm.numel()
    out = torch.empty(n, dtype=src.dtype, device=src.device)
    if n:
        nat.check(nat.load().hgd_gather32(src.data_ptr(), perm.data_ptr(), n, out.data_ptr(),
                                          _stream(src.device)), "hgd_gather32")
    return out


def _gather32_cached(cache: dict, kind: int, src: torch.Tensor,
                     perm: torch.Tensor) -> torch.Tensor:
    """``_gather32(src, perm)`` cached in ``cache`` under (kind, id(src)) while ``src`` is alive
    and unmodified (its version counter), e.g. the cached ``Incidence.edge_values`` a training
    step passes to every hop; the last 8 are kept."""
    try:
        version = src._version
    except RuntimeError:  # an inference tensor tracks no version: gathered every call
        return _gather32(src, perm)
    key = (kind, id(src))
    hit = cache.get(key)
    if hit is not None and hit[0]() is src and hit[1] == version:
        return hit[2]
    out = _gather32(src, perm)
    if len(cache) >= 8:
        cache.pop(next(iter(cache)))
    cache[key] = (weakref.ref(src), version, out)
    return out


def incidence_of(adj, cache: bool = True) -> Incidence:
    """The Incidence behind a torch sparse COO tensor (cached on the tensor object), or the
    argument itself when it already is one."""
    if isinstance(adj, Incidence):
        return adj
    inc = getattr(adj, "_hgd_incidence", None) if cache else None
    if (inc is not None and adj.layout == torch.strided
            and getattr(adj, "_hgd_incidence_version", None) != adj._version):
        inc = None  # a dense adjacency modified in place since its structure was taken
    if inc is None:
        if adj.layout == torch.sparse_coo:
            inc = Incidence.from_torch_sparse(adj)
        elif adj.layout == torch.strided and adj.dim() == 2:
            inc = Incidence.from_dense(adj)  # the pattern of a dense adjacency (DHCF)
        else:
            raise TypeError(f"incidence_of: unsupported adjacency layout {adj.layout}")
        if cache:
            try:
                adj._hgd_incidence = inc
                adj._hgd_incidence_version = adj._version
            except (AttributeError, RuntimeError):
                pass
    return inc
