"""MI355X-native hypergraph propagation for SELFRec-style recommenders.

The hot path — the incidence SpMM hops of HGNN / HCCF / ED-HNN ("hypergraph diffusion")
propagation and their backward — runs in hand-written gfx950 HIP kernels behind the C ABI of
``include/hgd.h`` (``_lib/libhgd.so``). The modules here sequence those calls and expose them
with the reference's operator signatures:

* :mod:`.incidence`  — device CSR/CSC structures (replaces per-call COO coalesce / ``adj.t()``)
* :mod:`.functional` — autograd hops: ``spmm``, ``two_hop``, ``hgconv2``, ``mean2hop``
* :mod:`.layers`     — drop-in ``GCNLayer``, ``HGNNLayer``, ``HGCNConv``, ``SpAdjDropEdge``,
                       ``EquivSetConv``, ``EquivSetGNN``, ``MLP``
* :mod:`.kg_attention` — KHGRec's per-batch KG attention (triple scores, row softmax) on device
* :mod:`.kg_loss`    — KHGRec's TransR KG loss, fused forward and backward (no [B, d, dr] gather)
* :mod:`.view_attention` — KHGRec's fusion of the two item views, one kernel each way
* :mod:`.cf_loss`    — KHGRec's CF loss (fusion + BPR + regulariser) over the batch's item rows only
* :mod:`.ingest`     — ``InteractionGraph`` / ``KnowledgeGraph``: the loaders' matrices and tables on device
* :mod:`.sampler`    — the reference's pairwise and unified (CF + KG) batches, bit for bit, in libhgd
* :mod:`.sharded`    — user-row sharding across GPUs with an RCCL all-reduce of hyperedge sums
"""
from . import _native
from .incidence import CSR, Incidence, incidence_of, spmm_csr, spmm_csr_fused_dt
from .functional import (att_two_hop, att_two_hop_fused, contrast_loss, hgconv2, mean2hop, spmm,
                         two_hop, unique_long)
from .kg_attention import KGAttentionPattern, kg_attention
from .kg_loss import kg_loss, kg_loss_rows
from .view_attention import view_attention, view_attention_stacked, view_attention_supported
from .cf_loss import cf_loss, cf_loss_supported
from .ingest import InteractionGraph, KnowledgeGraph

__all__ = ["InteractionGraph", "KnowledgeGraph","CSR", "Incidence", "incidence_of", "spmm_csr", "spmm", "two_hop", "hgconv2",
           "spmm_csr_fused_dt",
           "mean2hop", "contrast_loss", "unique_long", "att_two_hop", "att_two_hop_fused",
           "KGAttentionPattern", "kg_attention", "kg_loss", "kg_loss_rows", "view_attention",
           "view_attention_stacked", "view_attention_supported", "cf_loss", "cf_loss_supported",
           "_native"]
__version__ = "0.1.0"
