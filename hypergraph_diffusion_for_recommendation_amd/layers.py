"""Drop-in propagation layers with the reference's class names, constructor arguments and
``forward`` signatures (paths relative to /root/reference/HD_SELFRec).

Swapping ``from model.graph.HCCF import GCNLayer, HGNNLayer, SpAdjDropEdge`` (or the
``HGCNConv`` / ``EquivSetConv`` / ``EquivSetGNN`` / ``MLP`` classes) for these gives the same
outputs (fp32, 1e-5 relative) with every sparse hop on libhgd's gfx950 kernels:

=====================  ==============================================  =========================
class                  reference                                        hot op here
=====================  ==============================================  =========================
GCNLayer               model/graph/HCCF.py:193-199                      hgd_spmm (CSR, + CSC bwd)
HGNNLayer              model/graph/HCCF.py:201-211                      hgd_linear_* (f32 MFMA)
HGCNConv               model/graph/HGNN_HD4.py:450-462 (and copies)     2 hops, fused LeakyReLU
AttHGCNConv            model/graph/KHGRec.py:440-453                    4 hops, fused LeakyReLU
Attention              model/graph/KHGRec.py:466-480 (and copies)       hgd_view_attention_*
SpAdjDropEdge          model/graph/HCCF.py:213-226                      hgd_dropedge_compact
EquivSetConv           model/layers/layers2/EquivSetConv2.py:38-100     mean/sum 2-hop (V/E)
EquivSetGNN            model/layers/layers2/EquivSetGNN2.py:32-155      hgd_dense_threshold_*
MLP                    model/layers/MLP.py:29-117                       hgd_linear_* / row epi
=====================  ==============================================  =========================

Sparse adjacencies are accepted exactly as the reference passes them — torch sparse COO tensors
built by ``TorchGraphInterface.convert_sparse_mat_to_tensor`` — and converted once to a cached
device :class:`~.incidence.Incidence` (also accepted directly).
"""
from __future__ import annotations

import os
import time
import weakref
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .functional import (att_two_hop, dense_mean_two_hop, dense_mean_two_hop_ok,
                         dense_mean_two_hop_pair, dense_two_hop,
                         dropout_seed, layer_norm, linear, linear_relu_dropout, spmm, two_hop,
                         two_hop_fused)
from .incidence import (CSR, Incidence, MaskedIncidence, dense_threshold, drop_edges,
                        expand_rows, incidence_of)
from .view_attention import view_attention_stacked


class GCNLayer(nn.Module):
    """``torch.sparse.mm(adj, embeds)`` (HCCF.py:193-199; LeakyReLU constructed, unused, as
    in the reference)."""

    def __init__(self, leaky):
        super().__init__()
        self.act = nn.LeakyReLU(negative_slope=leaky)

    def forward(self, adj, embeds):
        return spmm(incidence_of(adj), embeds)


class HGNNLayer(nn.Module):
    """Dense learned hypergraph: ``adj·(adjᵀ·embeds)`` with adj = dropout(E·W) [n, K]
    (HCCF.py:201-211). K = hyper_dim (32): both products are skinny — the split-K and row
    MFMA kernels of hgd_linear_* (functional.dense_two_hop), forward and backward."""

    def __init__(self, leaky):
        super().__init__()
        self.act = nn.LeakyReLU(negative_slope=leaky)

    def forward(self, adj, embeds):
        return dense_two_hop(adj, embeds)


class HGCNConv(nn.Module):
    """``leaky(A·(Aᵀ·X))`` or ``A·(Aᵀ·X)`` (HGNN_HD4.py:450-462, HGCN.py:166-175,
    layers2/EquivSetConv2.py:104-117). No transpose is built per call: Aᵀ is the cached CSC."""

    def __init__(self, leaky):
        super().__init__()
        self.act = nn.LeakyReLU(negative_slope=leaky)

    def forward(self, adj, embs, act=True):
        inc = incidence_of(adj)
        if act:
            return two_hop(inc, embs, epilogue="leaky_relu", slope=self.act.negative_slope)
        return two_hop(inc, embs)


class AttHGCNConv(nn.Module):
    """KHGRec's attention conv (KHGRec.py:440-453): ``adj = att_adj·inp_adj`` and then
    ``leaky(adj·(adjᵀ·X))`` or ``adj·(adjᵀ·X)``. The reference forms ``adj`` with a sparse ×
    sparse product in every layer; here the same map runs as four hops,
    ``att·(K·(Kᵀ·(attᵀ·X)))`` (functional.att_two_hop), with neither the product nor its fill-in.

    ``inp_adj``: an Incidence, a torch sparse COO tensor or an edge-dropped view, as HGCNConv
    takes them. ``att_adj``: the Incidence of ``kg_attention`` / ``KGAttentionPattern.update``,
    or a torch sparse COO tensor such as the ``sparse_identity`` the reference starts with (its
    structure is rebuilt on every call, because the reference replaces that tensor's ``.data``
    in place). Gradient flows through ``embs`` only."""

    def __init__(self, leaky):
        super().__init__()
        self.act = nn.LeakyReLU(negative_slope=leaky)

    def forward(self, inp_adj, att_adj, embs, act=True):
        inc = incidence_of(inp_adj)
        att = incidence_of(att_adj, cache=False)
        if act:
            return att_two_hop(att, inc, embs, epilogue="leaky_relu",
                               slope=self.act.negative_slope)
        return att_two_hop(att, inc, embs)


_NATIVE_CPU_MASK: Optional[bool] = None


class Attention(nn.Module):
    """The view fusion of KHGRec.py:466-480 (the same class in HGNN_cp.py and HGNNAblation.py)
    with the reference's constructor and parameter names (``project.0.weight``,
    ``project.0.bias``, ``project.2.weight``: a reference ``state_dict`` loads). ``forward(z)``
    takes the stacked ``[N, 2, d]`` tensor and returns ``(fused, beta)``; on the device at a fused
    width it is one kernel forward and one backward (:func:`~.view_attention.view_attention`),
    anything else runs the reference's expression. ``beta`` carries no gradient (the reference's
    callers discard it); ``need_beta=False`` returns ``None`` in its place and skips building
    it. The two-tensor call without the stack is ``view_attention(z0, z1, *attention.weights())``.
    """

    def __init__(self, in_size, hidden_size=128, need_beta=True):
        super().__init__()
        if hidden_size != in_size:
            raise ValueError(f"Attention: hidden_size = {hidden_size} must equal in_size = "
                             f"{in_size}: the reference's (beta * z).sum(1) broadcasts beta "
                             f"[N, 2, hidden_size] against z [N, 2, in_size]")
        self.need_beta = bool(need_beta)
        self.project = nn.Sequential(
            nn.Linear(in_size, hidden_size),
            nn.Tanh(),
            nn.Linear(hidden_size, hidden_size, bias=False),
        )

    def weights(self):
        """``(weight1, bias1, weight2)`` as :func:`~.view_attention.view_attention` takes them."""
        return self.project[0].weight, self.project[0].bias, self.project[2].weight

    def forward(self, z):
        if self.need_beta:
            return view_attention_stacked(z, *self.weights(), return_beta=True)
        return view_attention_stacked(z, *self.weights()), None


def _native_cpu_mask_ok() -> bool:
    """Once per process: hgd_torch_cpu_keep_mask must reproduce torch.rand's mask and leave the
    generator where torch.rand leaves it (it restates torch's generator layout; if this torch
    build differs, torch.rand itself draws the mask)."""
    global _NATIVE_CPU_MASK
    if _NATIVE_CPU_MASK is None:
        from . import _native as nat
        saved = torch.get_rng_state()
        ok = saved.numel() == nat.load().hgd_torch_cpu_state_bytes()
        try:
            for n in (1, 623, 1250):
                if not ok:
                    break
                torch.set_rng_state(saved)
                ref = ((torch.rand(n) + 0.7).floor()).type(torch.bool)
                ref_next = torch.rand(4)
                torch.set_rng_state(saved)
                got, cnt = _native_keep_mask(n, 0.7)
                ok = bool((got.bool() == ref).all()) and cnt == int(ref.sum()) and bool(
                    (torch.rand(4) == ref_next).all())
        finally:
            torch.set_rng_state(saved)
        _NATIVE_CPU_MASK = ok
    return _NATIVE_CPU_MASK


# Host threads of a draw made ahead beside an eager step: the step's own launches are host-bound
# and need their core (16 draw threads on the GPU box's 16-CPU share took the HCCF eager step
# from 3.8 to 5.7 ms, profiles/r04_hccf/). Draws the caller waits for use the library default.
_EAGER_RNG_THREADS = int(os.environ.get("HGD_EAGER_RNG_THREADS", "8"))


def _draw_keep_mask(state: torch.Tensor, n: int, keep: float, threads: int = 0,
                    out: Optional[torch.Tensor] = None):
    """hgd_torch_cpu_keep_mask on a private copy of the generator state (advanced in place);
    ctypes drops the GIL for the call, so it can run on the prefetch thread. ``out``: a uint8
    host buffer of n bytes to draw into (else a new pinned one)."""
    import ctypes

    from . import _native as nat
    if out is not None and (out.dtype != torch.uint8 or out.numel() != n or out.is_cuda
                            or not out.is_contiguous()):
        raise ValueError("_draw_keep_mask: out must be a contiguous host uint8 buffer of n bytes")
    mask = out if out is not None else torch.empty(n, dtype=torch.uint8,
                                                   pin_memory=torch.cuda.is_available())
    kept = ctypes.c_int64(0)
    nat.check(nat.load().hgd_torch_cpu_keep_mask_threads(
        state.data_ptr(), state.numel(), n, float(keep), mask.data_ptr() if n else None,
        ctypes.byref(kept), int(threads)), "hgd_torch_cpu_keep_mask")
    return mask, int(kept.value), state


def _draw_step_masks(state: torch.Tensor, spec, threads: int = 0):
    """The masks of one step's drop calls ((n, keep) each, in order) from one generator state,
    advanced in place: [mask], state. Calls at one rate are ONE draw of Σn words split into
    views: ``torch.rand(n)`` takes exactly one generator word per element, so consecutive
    calls are consecutive stretches of one stream, and one split draw pays the threads'
    jump-ahead once instead of per call (HCCF: three 2.47 M masks per step)."""
    if len(spec) > 1 and len({keep for _, keep in spec}) == 1:
        total = sum(n for n, _ in spec)
        mask, _, state = _draw_keep_mask(state, total, spec[0][1], threads)
        masks, off = [], 0
        for n, _ in spec:
            masks.append(mask[off:off + n])
            off += n
        return masks, state
    masks = []
    for n, keep in spec:
        mask, _, state = _draw_keep_mask(state, n, keep, threads)
        masks.append(mask)
    return masks, state


_STEP_POOL = None


def _step_pool():
    global _STEP_POOL
    if _STEP_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _STEP_POOL = ThreadPoolExecutor(max_workers=1, thread_name_prefix="hgd-step-masks")
    return _STEP_POOL


def _native_keep_mask(n: int, keep: float):
    mask, kept, st = _draw_keep_mask(torch.get_rng_state(), n, keep)
    torch.set_rng_state(st)
    return mask, kept


# Masks of the same size and rate kept drawn ahead of the caller: the encoders make a step's
# drop calls back to back (HCCF: one per layer, before the layers run), so one mask ahead left
# the step's other draws in its critical path.
_KEEP_MASK_AHEAD = int(os.environ.get("HGD_KEEP_MASK_AHEAD", "3"))


class _KeepMaskPrefetcher:
    """Keeps the next ``_KEEP_MASK_AHEAD`` masks of the same size and rate drawn on a worker
    thread — a chain, each from the generator state the previous one leaves behind — while the
    caller launches its device work. A drawn-ahead mask is used only if the default generator is
    still exactly in the state it was drawn from (nothing else drew in between); otherwise the
    chain is discarded and the mask drawn there and then — so the stream stays the reference's
    either way."""

    def __init__(self):
        from concurrent.futures import ThreadPoolExecutor
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="hgd-keep-mask")
        self._chain = []     # futures of (start state, mask, kept, end state), in draw order
        self._key = None     # (n, keep) of the chain
        self._tail = None    # the state the last queued draw starts from: [tensor], worker-owned

    def _extend(self):
        tail, (n, keep) = self._tail, self._key

        def draw_next():  # jobs run in submission order on the one worker
            start = tail[0]
            mask, kept, end = _draw_keep_mask(start.clone(), n, keep, _EAGER_RNG_THREADS)
            tail[0] = end
            return start, mask, kept, end
        self._chain.append(self._pool.submit(draw_next))

    def _drop_chain(self):
        for f in self._chain:
            f.result()  # never leave a draw running behind a discarded one
        self._chain = []

    def get(self, n: int, keep: float):
        st = torch.get_rng_state()
        got = None
        if self._chain and self._key == (n, keep):
            start, mask, kept, end = self._chain.pop(0).result()
            if torch.equal(start, st):
                got = (mask, kept, end)
        if got is None:
            self._drop_chain()
            mask, kept, end = _draw_keep_mask(st, n, keep)
            got = (mask, kept, end)
            self._key, self._tail = (n, keep), [end.clone()]
        torch.set_rng_state(got[2])
        while len(self._chain) < _KEEP_MASK_AHEAD:
            self._extend()
        return got[0], got[1]


_PREFETCH: Optional[_KeepMaskPrefetcher] = None


def torch_cpu_keep_mask(n: int, keep: float, prefetch: bool = True):
    """``((torch.rand(n) + keep).floor()).type(torch.bool)`` of HCCF.py:223 on the default CPU
    generator — bit-identical mask and generator advance — as (uint8 host mask, kept count):
    one native pass split over threads by MT19937 jump-ahead (hgd_torch_cpu_keep_mask_threads;
    0.36–1.2 ms at 2.47 M entries) instead of torch's rand + add + floor + cast + count; with
    ``prefetch`` the next draws of the same shape are computed ahead on a worker thread
    (_KeepMaskPrefetcher; used only if the generator has not moved meanwhile)."""
    global _PREFETCH
    if _native_cpu_mask_ok():
        if not prefetch:
            return _native_keep_mask(n, keep)
        if _PREFETCH is None:
            _PREFETCH = _KeepMaskPrefetcher()
        return _PREFETCH.get(n, keep)
    mask = ((torch.rand(n) + keep).floor()).type(torch.bool)
    return mask, int(mask.sum())


class _MaskStager:
    """The next step's drop-edge masks on the device before its replay starts: the worker thread
    that draws them (SpAdjDropEdge.refill) draws into one of two pinned host buffers and copies
    it host → device into the matching device staging buffer on a side stream, so the transfer
    (7.4 MB per HCCF step, ~0.15 ms over PCIe) runs under the current replay instead of in front
    of the next one; the replay's stream then waits for that copy and moves the masks into the
    slots with one device-to-device pass. A pair of buffers is refilled only after the copies
    that read it (an event per buffer for each direction). The host buffers are the stager's own:
    a fresh pinned block per step left the caching host allocator allocating whenever the host
    ran a few steps ahead of the device (multi-millisecond stalls)."""

    def __init__(self, device, total: int):
        self.device = torch.device(device)
        self.total = int(total)
        self.bufs = [torch.empty(self.total, dtype=torch.uint8, device=self.device)
                     for _ in range(2)]
        self.host = [torch.empty(self.total, dtype=torch.uint8, pin_memory=True)
                     for _ in range(2)]
        self.free = [None, None]    # event: the slot copies that last read device buffer k
        self.copied = [None, None]  # event: the H2D copy that last read host buffer k
        self.next = 0
        self.side = torch.cuda.Stream(self.device)
        self.trace = None  # a list: per-job timings appended (scripts/profile_graph_step_host.py)

    def draw_and_stage(self, state: torch.Tensor, spec, target: Optional[torch.Tensor] = None,
                       target_free: Optional[torch.cuda.Event] = None):
        """(masks, end state, staged) on the worker thread: the step's masks drawn as one
        split draw into a host buffer and queued host → device on the side stream — into this
        stager's device buffer, or straight into ``target`` (a slot bank's buffer) once
        ``target_free`` (its last reader) has passed."""
        if not (len(spec) > 1 and len({keep for _, keep in spec}) == 1
                and sum(n for n, _ in spec) == self.total):
            masks, end = _draw_step_masks(state, spec)  # rates differ: per-call masks, copied
            return masks, end, None                     # in refill
        trace = self.trace
        t0 = time.perf_counter() if trace is not None else 0.0
        k = self.next
        self.next ^= 1
        if self.copied[k] is not None:
            self.copied[k].synchronize()  # its previous H2D copy has read it (long done)
        t1 = time.perf_counter() if trace is not None else 0.0
        host = self.host[k]
        _, _, end = _draw_keep_mask(state, self.total, spec[0][1], out=host)
        t2 = time.perf_counter() if trace is not None else 0.0
        masks, off = [], 0
        for n, _ in spec:
            masks.append(host[off:off + n])
            off += n
        torch.cuda.set_device(self.device)
        # the destination's last reader is waited for on this (worker) thread before the copy is
        # issued, not only by the side stream: on this stack gloo's staging copies, queued behind
        # a stream wait on a still-pending event, did not reliably see their producer's output
        # (the one-device rehearsals); here that order keeps a copy from overwriting
        # masks a queued replay still reads. The wait is for the step before last, so the copy
        # still runs under the next replay.
        free = target_free if target is not None else self.free[k]
        if free is not None:
            free.synchronize()
        with torch.cuda.stream(self.side):
            if free is not None:
                self.side.wait_event(free)
            (target if target is not None else self.bufs[k]).copy_(host, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.side)
        self.copied[k] = done
        if trace is not None:  # (host_wait, draw, stage) µs per job, for the profile scripts
            trace.append(((t1 - t0) * 1e6, (t2 - t1) * 1e6, (time.perf_counter() - t2) * 1e6))
        return masks, end, (k, done, host)

    def into_slots(self, staged, slots, flat=None) -> None:
        k, done, _host = staged
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(done)
        if flat is not None and flat.numel() == self.total:  # the slots are views of one buffer
            flat.copy_(self.bufs[k])
        else:
            off = 0
            for n, _, buf in slots:
                buf.copy_(self.bufs[k][off:off + n])
                off += n
        ev = torch.cuda.Event()
        ev.record(cur)
        self.free[k] = ev


class SpAdjDropEdge(nn.Module):
    """Edge dropout on a sparse COO adjacency (HCCF.py:213-226).

    By default the keep-mask is drawn exactly as the reference does — ``torch.rand(nnz)`` on the
    CPU generator, ``floor(rand + keepRate)`` — so it is bit-identical for the same seed.
    ``device_rng=True`` draws it on the GPU instead (hgd_bernoulli_mask, seeded from the CPU
    generator so ``torch.manual_seed`` still fixes it): same distribution, no host RNG / H2D.
    The compaction (``idxs[:, mask]``, ``vals[mask] / keepRate``) and the CSR/CSC of the result
    are built on the device; for the row-major COO of ``convert_sparse_mat_to_tensor`` the
    structure is derived from the parent's without sorting (Incidence.drop).
    """

    def __init__(self, device_rng: bool = False, capture_safe: bool = False):
        super().__init__()
        self.device_rng = device_rng
        # capture_safe: the result is a masked VIEW of the parent (Incidence.masked: the hops
        # skip the dropped edges, no compaction) and nothing is read back to the host, so the
        # step can be replayed from a HIP graph. The return value is then an Incidence (what
        # GCNLayer / HGCNConv consume), not a torch sparse COO. The mask comes either from a
        # device-side seed counter (device_rng: fresh masks every replay, a different stream)
        # or — the reference's own CPU torch.rand stream — from a static device buffer per call
        # of the step ("slot"), filled from the host: drawn inline on eager steps, and by
        # refill() before each replay once host_fed(True) is set.
        self.capture_safe = capture_safe
        self._seed = None
        self._slots = []       # [(nnz, keep, device uint8 buffer)] per call of a step
        self._slot_i = 0
        self._prefilled = False
        self._step_job = None  # (start state, spec, future, bank) of the next step's masks
        self._stage = None     # device staging of the next step's masks (refill)
        self._banks = []       # host_fed(banks=2): [(slots, flat buffer)] the refills alternate
        self._refills = 0      # refills so far (a step's bank is refills % len(banks))
        self._bank = 0         # the bank the slots are (0 without banks)

    def begin_step(self):
        """A step boundary: the next drop uses the first slot (encoders call it per forward)."""
        self._slot_i = 0

    def host_fed(self, on: bool = True, banks: int = 1):
        """capture_safe masks on the reference's CPU stream drawn ahead by :meth:`refill` (for a
        captured step, whose replays do not run Python) instead of inside the step. Turning it
        on (before the step is captured) also lays the step's slots out as consecutive views of
        one buffer, so a refill moves them with one device copy. ``banks=2`` keeps two such
        buffers that the refills alternate between (:meth:`use_bank` selects one for a capture):
        the draw worker copies a step's masks host → device straight into its bank while the
        previous step — on the other bank — runs, so no device-to-device pass is left between
        two replays (one captured step per bank)."""
        self._prefilled = bool(on)
        if on and len(self._slots) > 1:
            flat = getattr(self, "_slot_flat", None)
            total = sum(n for n, _, _ in self._slots)
            if flat is None or flat.numel() != total:
                flat = torch.empty(total, dtype=torch.uint8, device=self._slots[0][2].device)
                slots, off = [], 0
                for n, keep, buf in self._slots:
                    view = flat[off:off + n]
                    view.copy_(buf)
                    slots.append((n, keep, view))
                    off += n
                self._slots, self._slot_flat = slots, flat
                self._banks = []
            if banks == 2 and len(self._banks) != 2:
                flat2 = flat.clone()
                slots2, off = [], 0
                for n, keep, _ in self._slots:
                    slots2.append((n, keep, flat2[off:off + n]))
                    off += n
                self._banks = [(self._slots, flat), (slots2, flat2)]
                self._bank = 0

    def use_bank(self, b: int) -> None:
        """The slot bank the next drop calls read (a capture records that bank's buffers)."""
        self._slots, self._slot_flat = self._banks[b]
        self._bank = b

    def upcoming_bank(self) -> int:
        """The bank the next :meth:`refill` fills (0 without banks)."""
        return self._refills % len(self._banks) if self._banks else 0

    def refill(self):
        """Draws the next step's masks from the CPU generator — the same draws, in the same
        order, as the step's drop calls would make — into the slots' device buffers (copies
        ordered on the current stream before the step that reads them). The masks of the step
        after are then drawn on a worker thread while this one runs (all library threads: a
        replayed step leaves the host idle), and used only if nothing else moved the generator
        in between — the stream stays the reference's either way."""
        banked = len(self._banks) == 2
        if banked:
            self.use_bank(self._refills % 2)
        self._refills += 1
        spec = tuple((n, keep) for n, keep, _ in self._slots)
        staged = None
        cur = torch.cuda.current_stream(self._slots[0][2].device)
        if not _native_cpu_mask_ok():
            masks = [torch_cpu_keep_mask(n, keep, prefetch=False)[0] for n, keep in spec]
        else:
            st = torch.get_rng_state()
            job, self._step_job = getattr(self, "_step_job", None), None
            if job is not None and job[1] == spec and torch.equal(job[0], st) and (
                    not banked or job[3] == self._bank):
                masks, end, staged = job[2].result()
            else:
                if job is not None:
                    job[2].result()  # never leave a draw running behind a discarded one
                masks, end = _draw_step_masks(st, spec)
            torch.set_rng_state(end)
            stager = self._stager()
            target = free = None
            nxt = self._bank
            if banked:
                # the next step's bank was last read by the replay issued before this refill:
                # an event recorded now orders the worker's copy into it after that replay
                nxt = self._bank ^ 1
                target = self._banks[nxt][1]
                free = torch.cuda.Event()
                free.record(cur)
            self._step_job = (end.clone(), spec, _step_pool().submit(
                stager.draw_and_stage, end.clone(), spec, target, free), nxt)
        if staged is not None:
            if banked:  # already in this step's bank: the replay only waits for the copy
                cur.wait_event(staged[1])
            else:  # in the staging buffer: one D2D pass into the slots
                self._stage.into_slots(staged, self._slots, getattr(self, "_slot_flat", None))
        else:
            if banked and self._stage is not None:
                cur.wait_stream(self._stage.side)  # a discarded job's copy may target this bank
            for (n, keep, buf), mask in zip(self._slots, masks):
                buf.copy_(mask, non_blocking=True)
        self._slot_i = 0

    def _stager(self) -> "_MaskStager":
        dev = self._slots[0][2].device
        if self._stage is None or self._stage.device != dev:
            self._stage = _MaskStager(dev, sum(n for n, _, _ in self._slots))
        return self._stage

    def forward(self, adj, keepRate):
        if keepRate == 1.0:
            return adj
        if self.capture_safe:
            return self._capture_safe_drop(adj, float(keepRate))
        vals = adj._values()
        idxs = adj._indices()
        edgeNum = vals.size()
        device = vals.device if vals.device.type == "cuda" else torch.device("cuda")
        parent = incidence_of(adj) if vals.device.type == "cuda" else None
        if self.device_rng:
            from . import _native as nat
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            mask = torch.empty(edgeNum, dtype=torch.uint8, device=device)
            if mask.numel():
                nat.check(nat.load().hgd_bernoulli_mask(
                    seed, mask.numel(), float(keepRate), mask.data_ptr(),
                    nat.stream_handle(device)), "hgd_bernoulli_mask")
            count = None
        else:
            mask, count = torch_cpu_keep_mask(vals.numel(), keepRate)
            mask = mask.to(device, non_blocking=True)
        child = None
        if parent is not None and parent.coo_sorted and parent.perm_t is not None:
            # COO order == CSR order: the structure first (sized by the host count when the mask
            # was drawn on the host, else by its one device→host read), then the COO compaction
            child = parent.drop(mask, keepRate, kept=count)
            count = child.nnz
        new_idx, new_vals = drop_edges(idxs.to(device), vals.to(device), mask, keepRate, count)
        out = torch.sparse_coo_tensor(new_idx, new_vals, adj.shape)
        out._hgd_incidence = child if child is not None else Incidence.from_coo(
            new_idx, new_vals, adj.shape, device=device, validate=False)
        return out

    def _capture_safe_drop(self, adj, keep: float) -> "MaskedIncidence":
        from . import _native as nat
        parent = incidence_of(adj)
        if not (parent.coo_sorted and parent.perm_t is not None):
            raise RuntimeError("SpAdjDropEdge(capture_safe): needs a row-sorted base adjacency")
        dev = parent.device
        if not self.device_rng:  # the reference's CPU stream through this call's slot
            i = self._slot_i
            self._slot_i += 1
            if i == len(self._slots):
                if self._prefilled:
                    raise RuntimeError("SpAdjDropEdge: more drop calls in this step than the "
                                       "refilled slots (call begin_step per step)")
                self._slots.append((parent.nnz, keep,
                                    torch.empty(parent.nnz, dtype=torch.uint8, device=dev)))
            n, k, buf = self._slots[i]
            if n != parent.nnz or k != keep:
                raise RuntimeError("SpAdjDropEdge: a step's drop calls changed size or rate")
            if not self._prefilled:
                mask, _ = torch_cpu_keep_mask(n, keep)
                buf.copy_(mask, non_blocking=True)
            return parent.masked(buf, keep)
        if self._seed is None or self._seed.device != dev:
            # drawn once from the CPU generator (torch.manual_seed fixes the stream); advanced
            # on the device afterwards
            self._seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(dev)
        mask = torch.empty(parent.nnz, dtype=torch.uint8, device=dev)
        mask_t = torch.empty_like(mask)
        if parent.nnz:
            nat.check(nat.load().hgd_bernoulli_mask_dev_pair(
                self._seed.data_ptr(), parent.perm_t.data_ptr(), parent.nnz, keep,
                mask.data_ptr(), mask_t.data_ptr(), nat.stream_handle(dev)),
                "hgd_bernoulli_mask_dev_pair")
        self._seed.add_(1)
        return parent.masked(mask, keep, mask_t)


class Linear(nn.Linear):
    """nn.Linear (same parameters and state_dict) whose forward runs hgd_linear_* for the skinny
    shapes of the ED-HNN block (functional.linear); ``forward(x, relu=True)`` fuses the ReLU
    that follows lin_in and the hidden MLP layers."""

    def forward(self, x, relu: bool = False):
        return linear(x, self.weight, self.bias, relu)


class LayerNorm(nn.LayerNorm):
    """nn.LayerNorm (same parameters and state_dict) running hgd_row_epilogue_* for device fp32
    rows of up to 256 features (functional.layer_norm): one pass forward, one pass backward
    with the γ/β gradients, instead of the library's three kernels."""

    def forward(self, x):
        return layer_norm(x, self)


class MLP(nn.Module):
    """Same parameter layout and forward as model/layers/MLP.py:29-117 (adapted from
    CorrectAndSmooth): [norm] → (Linear → ReLU → norm → dropout)* → Linear."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout=.5,
                 Normalization='bn', InputNorm=False):
        super().__init__()
        self.in_channels = in_channels
        self.hidden_channels = hidden_channels
        self.out_channels = out_channels
        self.lins = nn.ModuleList()
        self.normalizations = nn.ModuleList()
        self.InputNorm = InputNorm
        assert Normalization in ['bn', 'ln', 'None']
        norm = {'bn': nn.BatchNorm1d, 'ln': LayerNorm, 'None': None}[Normalization]

        def mk(c):
            return norm(c) if norm is not None else nn.Identity()

        first = mk(in_channels) if (InputNorm and norm is not None) else nn.Identity()
        self.normalizations.append(first)
        if num_layers == 1:
            self.lins.append(Linear(in_channels, out_channels))
        else:
            self.lins.append(Linear(in_channels, hidden_channels))
            self.normalizations.append(mk(hidden_channels))
            for _ in range(num_layers - 2):
                self.lins.append(Linear(hidden_channels, hidden_channels))
                self.normalizations.append(mk(hidden_channels))
            self.lins.append(Linear(hidden_channels, out_channels))
        self.dropout = dropout

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()
        for n in self.normalizations:
            if not isinstance(n, nn.Identity):
                n.reset_parameters()

    def forward(self, x):
        x = self.normalizations[0](x)
        for i, lin in enumerate(self.lins[:-1]):
            x = lin(x, relu=True)  # Linear → ReLU fused
            x = self.normalizations[i + 1](x)
            x = F.dropout(x, p=self.dropout, training=self.training)
        return self.lins[-1](x)


def _relu_if(x: torch.Tensor, relu: bool) -> torch.Tensor:
    return F.relu(x) if relu else x


def input_norm_linear(W) -> Optional[tuple]:
    """(LayerNorm, Linear) when ``W`` is an :class:`MLP` of one Linear behind its InputNorm
    LayerNorm (HGNN_HD4's EquivSetConv.W: MLP3_num_layers 1, normalization 'ln', input_norm,
    HGNN_HD4.py:371-388) — the LayerNorm can then run in the store of the hop that feeds it."""
    if (isinstance(W, MLP) and len(W.lins) == 1 and W.InputNorm
            and isinstance(W.normalizations[0], LayerNorm)):
        return W.normalizations[0], W.lins[0]
    return None


def _position_incidence(index: torch.Tensor, n_out: int) -> Incidence:
    """P[index[k], k] = 1: scatter over nonzero positions (P·src) and, transposed, the gather
    src[index] (Pᵀ·X) — both as hgd_spmm hops."""
    k = torch.arange(index.numel(), device=index.device, dtype=torch.int64)
    return Incidence.from_coo(torch.stack([index.to(torch.int64), k]), None,
                              (n_out, index.numel()), device=index.device)


class EquivSetConv(nn.Module):
    """ED-HNN equivariant set convolution (layers2/EquivSetConv2.py:38-100).

    With W2 = the slice of the edge half (mlp2_layers = 0, HGNN_HD4's configuration) the
    vertex→edge→vertex aggregation is one fused two-hop over the binary V/E incidence:
    ``Xv = D_v^-1·B·D_e^-1·Bᵀ·W1(X)`` for 'mean' (torch_scatter's mean), without the
    [nnz, d] gathers the reference materialises. With an MLP W2 the per-nonzero concat path
    is kept (gather and scatter are hgd_spmm hops over position incidences).
    """

    def __init__(self, in_features, out_features, mlp1_layers=1, mlp2_layers=1, mlp3_layers=1,
                 aggr='add', alpha=0.5, dropout=0., normalization='None', input_norm=False,
                 hypergraph=None, data=None):
        super().__init__()
        if mlp1_layers > 0:
            self.W1 = MLP(in_features, out_features, out_features, mlp1_layers, dropout=dropout,
                          Normalization=normalization, InputNorm=input_norm)
        else:
            self.W1 = nn.Identity()
        self.in_features = in_features
        self.mlp2_layers = mlp2_layers
        if mlp2_layers > 0:
            self.W2 = MLP(in_features + out_features, out_features, out_features, mlp2_layers,
                          dropout=dropout, Normalization=normalization, InputNorm=input_norm)
        else:
            self.W2 = None  # X[..., in_features:] of the concat == the edge messages
        if mlp3_layers > 0:
            self.W = MLP(out_features, out_features, out_features, mlp3_layers, dropout=dropout,
                         Normalization=normalization, InputNorm=input_norm)
        else:
            self.W = nn.Identity()
        if aggr not in ('add', 'sum', 'mean'):
            raise ValueError(f"EquivSetConv: unsupported aggr {aggr!r}")
        self.aggr = aggr
        self.alpha = alpha
        self.dropout = dropout
        self.data = data
        self._cache = None
        self.fused_epilogue = True  # False: the reference's separate blend ops (A/B benches)

    def reset_parameters(self):
        for m in (self.W1, self.W2, self.W):
            if isinstance(m, MLP):
                m.reset_parameters()

    def _incidence(self, vertex, edges, N) -> Incidence:
        # V from EquivSetGNN.generate_V_E carries its incidence; otherwise cache by tensor
        # identity (weakrefs: an address or id() can be reused by a NEW tensor, e.g. the
        # per-step learned hypergraph of HCCF_diffusion.py:205-206, and must not hit)
        inc = getattr(vertex, "_hgd_incidence", None)
        if inc is not None and inc.n_rows == N:
            return inc
        c = self._cache
        if (c is not None and c[0]() is vertex and c[1]() is edges
                and c[2] == (int(N), vertex._version, edges._version)):
            return c[3]
        inc = Incidence.from_index_lists(vertex, edges, N)
        self._cache = (weakref.ref(vertex), weakref.ref(edges),
                       (int(N), vertex._version, edges._version), inc)
        return inc

    def forward(self, X, vertex, edges, X0, relu: bool = False):
        """``relu``: apply the ReLU that follows the conv in EquivSetGNN (its ``act``), fused
        into W's Linear where the fused path runs."""
        N = X.shape[-2]
        inc = self._incidence(vertex, edges, N)
        scale = "mean" if self.aggr == "mean" else None
        Xs = self.W1(X)
        if self.W2 is None:
            if self.alpha == 0 and self.fused_epilogue:
                # (1-0)·Xv + 0·X0 is Xv for finite X0 (HGNN_HD4's restart_alpha = 0): no blend,
                # no X0 read, and the plain two-hop's backward; W's InputNorm LayerNorm (MLP.py:
                # 109-110) runs in the second hop's store instead of its own [N, d] pass
                ln_lin = input_norm_linear(self.W)
                if ln_lin is not None:
                    return ln_lin[1](two_hop_fused(inc, Xs, P=scale, Q=scale, norm=ln_lin[0]),
                                     relu=relu)
                return _relu_if(self.W(two_hop(inc, Xs, P=scale, Q=scale, R=None)), relu)
            if self.fused_epilogue and torch.is_tensor(X0) and tuple(X0.shape) == (N, Xs.shape[1]):
                # restart blend (1-α)·Xv + α·X0 fused into the second hop's store
                return _relu_if(self.W(two_hop_fused(inc, Xs, P=scale, Q=scale,
                                                     out_scale=1 - self.alpha, res1=X0,
                                                     res1_scale=self.alpha)), relu)
            Xv = two_hop(inc, Xs, P=scale, Q=scale, R=None)
        else:
            # general path: Xe = aggr(W1(X)[V], E); Xv = aggr(W2([X[V], Xe[E]]), V)
            pos_v = self._pos(vertex, N, "v")
            pos_e = self._pos(edges, inc.n_cols, "e")
            Xve = spmm(pos_v, Xs, transpose=True)          # W1(X)[V]
            Xe = spmm(pos_e, Xve)                          # sum over E
            if scale:
                Xe = Xe * inc.scale("col", "mean")[:, None]
            Xev = spmm(pos_e, Xe, transpose=True)          # Xe[E]
            Xev = self.W2(torch.cat([spmm(pos_v, X, transpose=True), Xev], -1))
            Xv = spmm(pos_v, Xev)                          # sum over V
            if scale:
                Xv = Xv * inc.scale("row", "mean")[:, None]
        X = (1 - self.alpha) * Xv + self.alpha * X0
        return _relu_if(self.W(X), relu)

    def fused_tail_ok(self) -> bool:
        """The HGNN_HD4 configuration (restart_alpha 0, W2 the edge-half slice, W = InputNorm
        LayerNorm → one Linear): the conv ends in one Linear that can carry the block's ReLU,
        dropout and residual in its store (:meth:`forward_tail`)."""
        return (self.W2 is None and self.alpha == 0 and self.fused_epilogue
                and input_norm_linear(self.W) is not None)

    def forward_tail(self, X, vertex, edges, p: float, residual=None, seed=None):
        """``dropout(relu(conv(X)), p) (+ residual)`` for :meth:`fused_tail_ok` convs: the mean
        two-hop with W's LayerNorm in its store, then W's Linear with the ReLU, the dropout and
        the residual in its store (functional.linear_relu_dropout)."""
        N = X.shape[-2]
        inc = self._incidence(vertex, edges, N)
        scale = "mean" if self.aggr == "mean" else None
        ln, lin = input_norm_linear(self.W)
        y = two_hop_fused(inc, self.W1(X), P=scale, Q=scale, norm=ln)
        return linear_relu_dropout(y, lin.weight, lin.bias, p, res=residual, seed=seed)

    def _pos(self, index, n_out, tag):
        attr = f"_pos_{tag}"
        c = getattr(self, attr, None)
        if c is not None and c[0]() is index and c[1] == (index._version, n_out):
            return c[2]
        inc = _position_incidence(index.to(torch.device("cuda") if index.device.type != "cuda"
                                           else index.device), n_out)
        setattr(self, attr, (weakref.ref(index), (index._version, n_out), inc))
        return inc


class EquivSetGNN(nn.Module):
    """ED-HNN block (layers2/EquivSetGNN2.py:32-155): dropout → ReLU(lin_in) → x0 →
    [dropout → EquivSetConv → act] × All_num_layers → dropout.

    ``generate_V_E`` is ``torch.nonzero(hypergraph > 0)`` done on the device with
    hgd_dense_threshold_* (identical row-major order) and cached per hypergraph object, instead
    of two O(N²) CPU scans + H2D per call. A torch sparse COO or an :class:`Incidence` is also
    accepted as ``hypergraph``.
    """

    def __init__(self, num_features, args, dense_hypergraph=None, data=None):
        super().__init__()
        act = {'Id': nn.Identity(), 'relu': nn.ReLU(), 'prelu': nn.PReLU()}
        self.act = act[args['activation']]
        self.input_drop = nn.Dropout(args['input_dropout'])
        self.dropout = nn.Dropout(args['dropout'])
        self.data = data
        self.in_channels = num_features
        self.hidden_channels = args['MLP_hidden']
        self.mlp1_layers = args['MLP_num_layers']
        self.mlp2_layers = (args['MLP_num_layers'] if args['MLP2_num_layers'] < 0
                            else args['MLP2_num_layers'])
        self.mlp3_layers = (args['MLP_num_layers'] if args['MLP3_num_layers'] < 0
                            else args['MLP3_num_layers'])
        self.nlayer = args['All_num_layers']
        self.lin_in = Linear(num_features, args['MLP_hidden'])
        self.conv = EquivSetConv(args['MLP_hidden'], args['MLP_hidden'],
                                 mlp1_layers=self.mlp1_layers, mlp2_layers=self.mlp2_layers,
                                 mlp3_layers=self.mlp3_layers, alpha=args['restart_alpha'],
                                 aggr=args['aggregate'], dropout=args['dropout'],
                                 normalization=args['normalization'],
                                 input_norm=args['AllSet_input_norm'],
                                 hypergraph=dense_hypergraph, data=data)
        self._ve_cache = None
        # False: the module path (torch dropouts, separate ReLU / residual); True runs HGNN_HD4's
        # block with the library dropout in the Linear stores (same distribution, own RNG)
        self.fused_dropout = True

    def reset_parameters(self):
        self.lin_in.reset_parameters()
        self.conv.reset_parameters()

    def forward(self, x, hypergraph, n_nodes, residual=None):
        """``residual``: added to the block's output (LocalAwareEncoder's ``+ res``,
        HGNN_HD4.py:399) — in the last Linear's store when the fused path runs."""
        if (self._fused_dropout_ok() and self.conv.aggr == 'mean' and torch.is_tensor(hypergraph)
                and hypergraph.layout == torch.strided and dense_mean_two_hop_ok(hypergraph, x)
                and hypergraph.shape[0] == x.shape[0]):
            # a dense learned hypergraph (HCCF_diffusion.py:205-206): the mean pair straight
            # from H (functional.dense_mean_two_hop), no V/E lists and no host read
            p = self.dropout.p if self.training else 0.0
            seeds = [dropout_seed(x.device) for _ in range(3)] if p > 0.0 else [None] * 3
            # the input dropout rides in lin_in's operand load (never materialised)
            x = linear_relu_dropout(x, self.lin_in.weight, self.lin_in.bias, p, seed=seeds[1],
                                    in_p=p, in_seed=seeds[0])
            ln, lin = input_norm_linear(self.conv.W)
            y = layer_norm(dense_mean_two_hop(hypergraph, self.conv.W1(x)), ln)
            return linear_relu_dropout(y, lin.weight, lin.bias, p, res=residual, seed=seeds[2])
        V, E = self.generate_V_E(n_nodes, hypergraph)
        if self._fused_dropout_ok():
            # HGNN_HD4's block: every dropout on the library RNG (functional.dropout), the
            # second one in lin_in's store, the last one and the residual in W's store
            p = self.dropout.p if self.training else 0.0
            seeds = [dropout_seed(x.device) for _ in range(3)] if p > 0.0 else [None] * 3
            # the input dropout rides in lin_in's operand load (never materialised)
            x = linear_relu_dropout(x, self.lin_in.weight, self.lin_in.bias, p, seed=seeds[1],
                                    in_p=p, in_seed=seeds[0])
            return self.conv.forward_tail(x, V, E, p, residual=residual, seed=seeds[2])
        x = self.dropout(x)
        x = self.lin_in(x, relu=True)  # F.relu(lin_in(x)) fused
        x0 = x
        relu = isinstance(self.act, nn.ReLU)  # fused into the conv's last Linear when it can
        for _ in range(self.nlayer):
            x = self.dropout(x)
            x = self.conv(x, V, E, x0, relu=relu)
            if not relu:
                x = self.act(x)
        x = self.dropout(x)
        return x if residual is None else x + residual

    def dense_pair_ok(self, x, H_u, H_i) -> bool:
        """:meth:`forward_dense_pair` applies: the fused block, dense device hypergraphs over the
        two row blocks of ``x``; the dense pair computes the MEAN two-hop, so only a 'mean'
        aggregation takes it (an 'add' / 'sum' block runs the V/E path)."""
        return (self._fused_dropout_ok() and self.conv.aggr == 'mean'
                and torch.is_tensor(H_u) and torch.is_tensor(H_i)
                and H_u.layout == torch.strided and H_i.layout == torch.strided
                and H_u.shape[0] + H_i.shape[0] == x.shape[0] and H_u.shape[1] == H_i.shape[1]
                and x.is_contiguous() and x.shape[0] * x.shape[1] < 2 ** 32
                and dense_mean_two_hop_ok(H_u, x[:H_u.shape[0]])
                and dense_mean_two_hop_ok(H_i, x[H_u.shape[0]:]))

    def forward_dense_pair(self, x, H_u, H_i):
        """``cat([self(x[:nu], H_u, ·), self(x[nu:], H_i, ·)])`` (HCCF_diffusion.py:213-218: the
        block on the user rows with the user hypergraph, on the item rows with the item one) as
        ONE pass over all N rows: the row-wise stages (dropouts, lin_in, W1, LayerNorm, the last
        Linear) are one launch each on [N, d] and the two mean two-hops one grouped op
        (functional.dense_mean_two_hop_pair), the output written whole (no cat, no split of its
        gradient). Each dropout is one library-RNG mask over the [N, d] rows (same distribution
        as two per-half masks)."""
        p = self.dropout.p if self.training else 0.0
        seeds = [dropout_seed(x.device) for _ in range(3)] if p > 0.0 else [None] * 3
        x = linear_relu_dropout(x, self.lin_in.weight, self.lin_in.bias, p, seed=seeds[1],
                                in_p=p, in_seed=seeds[0])
        ln, lin = input_norm_linear(self.conv.W)
        y = layer_norm(dense_mean_two_hop_pair(H_u, H_i, self.conv.W1(x)), ln)
        return linear_relu_dropout(y, lin.weight, lin.bias, p, seed=seeds[2])

    def _fused_dropout_ok(self) -> bool:
        # exactly nn.Dropout (a test's recorded-mask dropout takes the module path), one conv
        # with the fused tail (x0 unused at restart_alpha 0), ReLU activation, device input
        return (type(self.dropout) is nn.Dropout and self.nlayer == 1
                and isinstance(self.act, nn.ReLU) and self.fused_dropout
                and isinstance(self.conv, EquivSetConv) and self.conv.fused_tail_ok()
                and 0.0 <= self.dropout.p < 1.0)

    def generate_V_E(self, n_nodes, hypergraph):
        """V = rows, E = cols of nonzero(hypergraph > 0), row-major (EquivSetGNN2.py:105-133)."""
        # cached per hypergraph OBJECT (weakref identity + version): the reference rebuilds V/E
        # on every call, and a learned hypergraph (HCCF_diffusion.py:205-206) is a new tensor
        # each step, whose id() may equal a dead predecessor's
        version = getattr(hypergraph, "_version", 0)
        c = self._ve_cache
        if c is not None and c[0]() is hypergraph and c[1] == version:
            return c[2]
        device = torch.device("cuda")
        if isinstance(hypergraph, Incidence):
            inc = hypergraph
            rowptr, cols = inc.csr.rowptr, inc.csr.col
        elif hypergraph.layout == torch.sparse_coo:
            h = hypergraph.to(device).coalesce()
            keep = h._values() > 0
            idx = h._indices()[:, keep]
            inc = Incidence.from_coo(idx, None, h.shape, device=device, rows_sorted=True)
            rowptr, cols = inc.csr.rowptr, inc.csr.col
        else:
            dense = hypergraph.to(device=device, dtype=torch.float32)
            rowptr, cols = dense_threshold(dense, 0.0)
            inc = None
        nnz = int(cols.numel())
        V = expand_rows(rowptr, nnz).to(torch.int64)
        E = cols.to(torch.int64)
        if inc is None:
            n_e = int(hypergraph.shape[1])
            csr_rows = V.to(torch.int32)
            inc = Incidence._from_sorted(csr_rows, cols, None, int(hypergraph.shape[0]), n_e)
        # E spans max(E)+1 hyperedges in the reference (torch_scatter's output size); extra empty
        # columns of the incidence contribute nothing, so the cached incidence is reused as is.
        V._hgd_incidence = inc
        self._ve_cache = (weakref.ref(hypergraph), version, (V, E))
        return V, E
