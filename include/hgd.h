/*
 * hgd.h — C ABI of libhgd, the MI355X (gfx950) hypergraph-propagation library.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json `north_star`:
 * the incidence SpMM hops (Hᵀ·X then H·M, with degree normalisation) that sit under
 * SELFRec's model/graph plugins, plus the per-step structure work feeding them.
 * Every entry point replaces one implicit device-op call site of the reference
 * (paths relative to /root/reference/HD_SELFRec):
 *
 *   hgd_spmm                 torch.sparse.mm(adj, X)            model/graph/HCCF.py:199,
 *                            torch.sparse.mm(adj.t(), X)        model/graph/HGNN_HD4.py:459-462,
 *                                                               model/graph/HGCN.py:173-175,
 *                            torch_scatter.scatter(.., 'mean')  model/layers/layers2/EquivSetConv2.py:88-93
 *                            (row_scale = 1/count is the scatter-mean; val = per-nonzero weight)
 *   hgd_spmm_dt              the same hops over bfloat16 tables (X and / or Y in 16 bits, fp32 sums)
 *   hgd_spmm_fused_dt        hgd_spmm_fused (the hop with the LayerNorm / residual row epilogue in
 *                            its store) gathering from a bfloat16 table
 *   hgd_row_epilogue_backward_dt  that epilogue's backward with dZ stored in bfloat16, for
 *                            backward hops that gather 16-bit tables
 *   hgd_spmm_blocked         the same torch.sparse.mm(adj.t(), X) hop for a gathered table larger
 *                            than the Infinity Cache (source-blocked; hgd_spmm_col_blocks builds
 *                            its block-major copy of the CSC)
 *   hgd_spmm_blocked_dt      the source-blocked hop over bfloat16 tables
 *   hgd_spmm_blocked_ordered the source-blocked hop with each block's rows walked in ascending
 *                            order of their first column (hgd_spmm_col_blocks_ordered builds it)
 *   hgd_spmm_blocked_packed  hgd_spmm_blocked_ordered over one packed word per nonzero (block-local
 *                            column + weight code), for weights expanded from a per-row scale
 *   hgd_spmm_blocked_split   the source-blocked hop over a structure with split rows (a split
 *                            plan per source block)
 *   hgd_sort_perm            COO→CSR / CSR→CSC ordering that cuSPARSE re-derives per call
 *                            (`adj.t()` in HGCNConv.forward, HGNN_HD4.py:459; coalesce in torch.sparse.mm)
 *   hgd_rowptr_from_sorted   row pointer of a row-sorted COO  base/torch_interface.py:8-12
 *   hgd_degree_scale         D^-1/2 and D^-1 of data/graph.py:11-25 (inf→0) and data/graph.py:28-42
 *   hgd_edge_values          per-nonzero weights with a source-side diagonal folded in
 *   hgd_dropedge_compact     SpAdjDropEdge.forward, model/graph/HCCF.py:213-226 (vals[mask]/keep, idxs[:,mask])
 *   hgd_dense_threshold_*    torch.nonzero(hypergraph > 0), model/layers/layers2/EquivSetGNN2.py:105-133
 *                            (row-major order identical to torch.nonzero)
 *   hgd_kg_attention_scores  update_attention_batch and its per-relation loop,
 *                            model/graph/KHGRec.py:298-320
 *   hgd_kg_attention_softmax torch.sparse.softmax(A_in.cpu(), dim=1), KHGRec.py:326-331
 *   hgd_kg_loss_forward      calculate_kg_loss, KHGRec.py:347-365 (trans_M[r], three torch.bmm,
 *                            logsigmoid, l2_reg_loss; also HD.py:371, HD2.py:368)
 *   hgd_kg_loss_backward     its autograd backward (the [B, d, dr] gradient and its index_put)
 *   hgd_kg_expand            Knowledge.construct_data's triple table, data/knowledge.py:44-72
 *   hgd_sample_unified       next_batch_unified, util/sampler.py:7-90 (host)
 *
 * Conventions:
 *   - All pointers are DEVICE pointers unless a parameter says "host".
 *   - The caller owns every buffer; the library never allocates or frees caller memory.
 *     Scratch comes from a caller-provided workspace sized by the matching *_workspace_size.
 *   - Every call is stream-ordered on `stream` (a hipStream_t passed as void*; NULL = legacy
 *     default stream) and performs no host synchronisation, so it can be graph-captured.
 *   - Errors come back as hgd_status; hgd_get_last_error_string() describes the last failure
 *     on the calling thread. No C++ exception crosses the ABI.
 *   - Indices: row pointers are int64, column/row indices are int32 (rows, cols < 2^31).
 *   - Floating point is fp32 in and out (hgd_spmm_dt / hgd_spmm_masked_dt / hgd_spmm_blocked_dt /
 *     hgd_spmm_fused_dt / hgd_spmm_masked_fused_dt also take bfloat16 tables, and
 *     hgd_row_epilogue_backward_dt writes one); sums run in fp32 in edge order (deterministic).
 */
#ifndef HGD_H
#define HGD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hgd_status {
  HGD_OK = 0,
  HGD_ERR_INVALID_ARG = 1,
  HGD_ERR_HIP = 2,
  HGD_ERR_UNSUPPORTED = 3,
  HGD_ERR_WORKSPACE = 4
} hgd_status;

typedef enum hgd_epilogue {
  HGD_EPI_NONE = 0,
  HGD_EPI_LEAKY_RELU = 1, /* nn.LeakyReLU(negative_slope=slope): HGCNConv act=True */
  HGD_EPI_RELU = 2
} hgd_epilogue;

/* Tuning knobs of the SpMM hop (process-wide; defaults are the measured best on MI355X).
 *   HGD_TUNE_SPMM_UNROLL: independent row gathers in flight per lane (8 or 16)
 *   HGD_TUNE_SPMM_POLICY: 0 plain, 1 non-temporal Y stores, 8 software-pipelined index
 *                         batches (default), 9 both, 10 prefetch + non-temporal index/weight
 *                         loads, 11 all three (d = 64 float4 path only)
 *   HGD_TUNE_SPMM_PASS_COLS: widest column pass of a hop without a fused row epilogue
 *                         (64, 128 or 256 fp32 columns; wider rows run as several passes;
 *                         0 = auto, the default: one pass up to 128 columns, else 64)
 *   HGD_TUNE_ROWGEMM_BLOCKS: most workgroups of a row-GEMM launch (hgd_gemm_rows, hgd_linear_*;
 *                         0 = default 512, else 64..8192; each wave takes 16-row tiles at a
 *                         stride of 4·blocks)
 *   HGD_TUNE_SPLITK_ROWS: rows per slice of the split-K products (hgd_gemm_tn,
 *                         hgd_linear_backward_weight; 0 = default sizing, else a multiple of 64
 *                         in [64, 65536]; the workspace size follows it)
 *   HGD_TUNE_GEMM_EXACT:  0 (default) = the dense products with K (row GEMM) or the row count's
 *                         reduction (split-K) eligible run as split-bf16 MFMAs (every f32
 *                         operand cut exactly into three bf16 terms, six products: error
 *                         ≈ 1e-7·Σ|a·b| like the f32 fmaf chain, not bitwise equal to it);
 *                         1 = the exact f32-input MFMA kernels only (bitwise k-ordered fmaf)
 *   HGD_TUNE_X3_COLS:     output columns per workgroup of the split-bf16 row GEMM (64 or 128;
 *                         0 = default)
 *   HGD_TUNE_X3_SPLITK:   weight-gradient (split-K) kernel when HGD_TUNE_GEMM_EXACT is 0:
 *                         2 (default) = by shape: the producer-wave split-bf16 kernel for
 *                         64 × 64 and 128 × 128 outputs (16-byte aligned rows, ≥ 4,096 rows),
 *                         the one-wave-per-tile split-bf16 kernel for other outputs ≤ 64 × 64
 *                         over ≥ 49,152 rows, else the f32-MFMA kernel; 1 = always the
 *                         one-wave-per-tile split-bf16 kernel; 0 = always f32 MFMA
 *   HGD_TUNE_X3S_TILES:   form of the staged split-bf16 row GEMM at N > 32: 1 or 2 16-column
 *                         tiles per wave (1: half the W registers, two workgroups per CU), 3 =
 *                         two tiles + 4 producer waves that load and split the rows while the
 *                         others multiply; 0 = default (1 for masked products, else 3)
 *   HGD_TUNE_P2P_SEGMENT_MB: largest allocation hgd_p2p_create exposes to its peers, in MiB
 *                         (0 = default 1024; slots are packed whole into segments of at most
 *                         this size, each imported separately: a single 3.5 GiB import never
 *                         returned on the ROCm 7.2 box); applies to later hgd_p2p_create calls
 *   HGD_TUNE_P2P_CACHED:  0 (default) = uncached segments (hipDeviceMallocUncached); 1 = plain
 *                         device memory (the exchange's fences keep it correct either way; the
 *                         knob prices what uncached hop-1 stores cost)
 *   HGD_TUNE_CPU_RNG_THREADS: host threads of hgd_torch_cpu_keep_mask's split draw (0 = default
 *                         min(16, hardware threads, OMP_NUM_THREADS); 1 = one thread)
 *   HGD_TUNE_X3P_QUEUE:   form of the producer-wave weight gradient: 0 (default) = one workgroup
 *                         barrier per 32-row stage, 1 = three LDS buffers with full / empty
 *                         counters (measured slower: 45.1 vs 41.5 µs at 144,242 x 128); a
 *                         counter wait that runs out (≈ 0.1 s) writes the workgroup's partial
 *                         sums as NaN instead of reading an unfilled buffer
 *   HGD_TUNE_P2P_GRID:    workgroups of the peer exchange's reduce / gather kernels (0 = default
 *                         256: the links bound them, the hops they overlap need the CUs)
 *   HGD_TUNE_MASK_PAIR:   the masked hop (hgd_spmm_masked*) walks two index batches per step,
 *                         their kept entries packed by forward permutes (2, default) or by
 *                         set-bit searches and pulls (1), or one batch per step (0); the sums
 *                         are the same bits every way
 *   HGD_TUNE_MASK_DIV:    the masked hop's kept weights val / keep: 0 (default) = one multiply by
 *                         1 / keep when keep is a power of two (the same bits: one real value,
 *                         rounded once), else the IEEE division; 1 = always the division
 *   HGD_TUNE_SPMM_PASS_INTERLEAVE: rows wider than one column pass (d > 128 by default, unfused,
 *                         no split rows): 0 = one launch per pass; 1 = all passes in one launch,
 *                         a row block's passes on consecutive workgroups of one XCD (the same
 *                         bits either way)
 *   HGD_TUNE_SPMM_BLOCKED_SEG: hgd_spmm_blocked walks each source block's (short) rows with
 *                         0 = a lane group per row (default), 1 = the segmented kernel (a group
 *                         owns G consecutive rows as one nonzero stream; the same bits) */
typedef enum hgd_tune_key {
  HGD_TUNE_SPMM_UNROLL = 1,
  HGD_TUNE_SPMM_POLICY = 2,
  HGD_TUNE_SPMM_PASS_COLS = 3,
  HGD_TUNE_ROWGEMM_BLOCKS = 4,
  HGD_TUNE_SPLITK_ROWS = 5,
  HGD_TUNE_GEMM_EXACT = 6,
  HGD_TUNE_X3_COLS = 7,
  HGD_TUNE_X3_SPLITK = 8,
  HGD_TUNE_X3S_TILES = 9,
  HGD_TUNE_P2P_SEGMENT_MB = 10,
  HGD_TUNE_P2P_CACHED = 11,
  HGD_TUNE_CPU_RNG_THREADS = 12,
  HGD_TUNE_X3P_QUEUE = 13,
  HGD_TUNE_P2P_GRID = 14,
  HGD_TUNE_MASK_PAIR = 15,
  HGD_TUNE_MASK_DIV = 16,
  HGD_TUNE_SPMM_PASS_INTERLEAVE = 17,
  HGD_TUNE_SPMM_BLOCKED_SEG = 18
} hgd_tune_key;
hgd_status hgd_set_tuning(int32_t key, int32_t value);

/* Library ABI version (major*10000 + minor*100 + patch). */
int hgd_version(void);
/* Human-readable description of the last error on this thread ("" if none). */
const char* hgd_get_last_error_string(void);

/* ------------------------------------------------------------------------------------------
 * Split plan for long rows. Rows whose degree exceeds `threshold` are cut into chunks of
 * `chunk` nonzeros, summed by separate wavefront groups into a workspace, then combined in
 * chunk order (deterministic, no atomics). All arrays are device arrays built by
 * hgd_split_plan_build; a NULL plan or n_heavy == 0 means no row is split.
 * ---------------------------------------------------------------------------------------- */
typedef struct hgd_split_plan {
  int64_t threshold;           /* rows with degree > threshold are split (<=0: none)   */
  int32_t chunk;               /* nonzeros per chunk                                    */
  int32_t flags;               /* HGD_PLAN_SEGMENTED: short rows, use the segmented kernel */
  int64_t n_heavy;             /* number of split rows                                  */
  int64_t n_chunks;            /* total chunks over all split rows                      */
  const int32_t* heavy_rows;   /* [n_heavy]   split row ids, ascending                  */
  const int64_t* heavy_cptr;   /* [n_heavy+1] chunk range of each split row             */
  const int32_t* chunk_heavy;  /* [n_chunks]  split-row index owning each chunk         */
} hgd_split_plan;

/* plan.flags bit: the structure has short rows (average degree ≲ 32) and no split rows —
 * hgd_spmm then walks groups of consecutive rows as one nonzero stream (segmented kernel). */
#define HGD_PLAN_SEGMENTED 1

/* Counts (n_heavy, n_chunks) for a plan into device int64[2] `counts`. */
hgd_status hgd_split_plan_count(const int64_t* rowptr, int64_t n_rows, int64_t threshold,
                                int32_t chunk, int64_t* counts, void* stream);
size_t hgd_split_plan_workspace_size(int64_t n_rows);
/* Fills plan->heavy_rows / heavy_cptr / chunk_heavy (caller-allocated, sized from counts). */
hgd_status hgd_split_plan_build(const int64_t* rowptr, int64_t n_rows, int64_t threshold,
                                int32_t chunk, int32_t* heavy_rows, int64_t* heavy_cptr,
                                int32_t* chunk_heavy, int64_t n_heavy, int64_t n_chunks,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * One SpMM hop over a CSR structure (the CSC of H is the CSR of Hᵀ):
 *   for r in [row_begin, row_end):
 *     Y[r, 0:d] = epi( row_scale[r] * Σ_{e=rowptr[r]}^{rowptr[r+1]-1} val[e] * X[col[e], 0:d] )
 * val == NULL means all ones; row_scale == NULL means 1. X rows are n_src_rows × ldx floats.
 * Rows outside [row_begin,row_end) are not written. Workspace: hgd_spmm_workspace_size.
 * ---------------------------------------------------------------------------------------- */
size_t hgd_spmm_workspace_size(const hgd_split_plan* plan, int32_t d);
hgd_status hgd_spmm(const int64_t* rowptr, const int32_t* col, const float* val,
                    const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                    int64_t row_begin, int64_t row_end, const float* X, int64_t ldx, float* Y,
                    int64_t ldy, int32_t d, int32_t epilogue, float slope,
                    const hgd_split_plan* plan, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * The same hop over tables stored in bfloat16. Replaces the same call sites as hgd_spmm
 * (torch.sparse.mm(adj, X), model/graph/HCCF.py:199; torch.sparse.mm(adj.t(), X),
 * model/graph/HGNN_HD4.py:459-462, model/graph/HGCN.py:173-175) when the embedding table is kept
 * or staged in 16 bits: the gathered rows are nnz·2d of the hop's bytes instead of nnz·4d.
 *   x_dtype / y_dtype: element type of X / Y (HGD_DT_F32 or HGD_DT_BF16); ldx / ldy count
 *   elements of their own type. Pairs: bf16→bf16, bf16→f32, f32→bf16, and f32→f32, which forwards
 *   to hgd_spmm / hgd_spmm_masked (bitwise theirs).
 * A bf16 element is widened to fp32 exactly; the sum is hgd_spmm's (one fp32 fmaf chain in edge
 * order, fp32 weights, row scales, split-row partials and activation); a bf16 Y is the fp32 result
 * rounded to nearest even — the one new rounding. Workspace: hgd_spmm_workspace_size (unchanged:
 * the partials are fp32). The 16-byte path needs d % 8 == 0 and 16-byte aligned rows on both sides
 * (ld % 8 == 0 for bf16, % 4 for fp32); other shapes take the scalar path.
 * ---------------------------------------------------------------------------------------- */
#define HGD_DT_F32 0
#define HGD_DT_BF16 1
hgd_status hgd_spmm_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                       const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                       int64_t row_begin, int64_t row_end, const void* X, int32_t x_dtype,
                       int64_t ldx, void* Y, int32_t y_dtype, int64_t ldy, int32_t d,
                       int32_t epilogue, float slope, const hgd_split_plan* plan, void* workspace,
                       size_t workspace_bytes, void* stream);
/* hgd_spmm_masked (the edge-dropped view: mask, keep) with the same element types. */
hgd_status hgd_spmm_masked_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                              const uint8_t* mask, float keep, const float* row_scale,
                              int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                              int64_t row_end, const void* X, int32_t x_dtype, int64_t ldx,
                              void* Y, int32_t y_dtype, int64_t ldy, int32_t d, int32_t epilogue,
                              float slope, const hgd_split_plan* plan, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same hop (rows [row_begin,row_end), no split plan) run in n_blocks passes over SOURCE-ROW
 * ranges [⌊n_src_rows·k/n_blocks⌋, ⌊n_src_rows·(k+1)/n_blocks⌋): pass k sums only a row's
 * nonzeros whose column lies in block k and adds that partial to Y (pass 0 writes it; the
 * activation runs after the last). Replaces the same call sites as hgd_spmm
 * (torch.sparse.mm(adj.t(), X), model/graph/HGNN_HD4.py:459-462) when the gathered table is too
 * large for the 256 MB Infinity Cache: each pass gathers from a 1/n_blocks slice of X, for
 * (n_blocks−1) extra read+write passes over Y. The sum is a different fp32 association of the same
 * terms (blockwise partials, each scaled by row_scale), so it is not bitwise hgd_spmm's.
 *
 * hgd_spmm_col_blocks builds the BLOCK-MAJOR copy of a structure whose rows' columns ascend (the
 * CSC of an incidence): all rows' block-0 nonzeros, then all rows' block-1 nonzeros, …
 *   blk_start: int64 [n_blocks·n_rows + 1], row r's block-k nonzeros are
 *              [blk_start[k·n_rows + r], blk_start[k·n_rows + r + 1]) of
 *   blk_col:   int32 [nnz], their columns, and
 *   blk_perm:  int32 [nnz] (may be NULL), their positions in the source structure — gather any
 *              per-nonzero weights through it (hgd_gather32) to get hgd_spmm_blocked's blk_val
 *              (int32 positions: nnz < 2^31, the library's limit for permutations, as perm_t).
 * Workspace: hgd_spmm_col_blocks_workspace_size.
 * ---------------------------------------------------------------------------------------- */
/* The size rule both hosts use (measured on MI355X): the number of source
 * blocks for a hop gathering n_src_rows rows at width d (a pass of at most 128 columns):
 * 0 (one pass) under 512 MiB, 2 under 1 GiB, else about one per 640 MiB, 4..16. */
int32_t hgd_spmm_blocks_for(int64_t n_src_rows, int32_t d);
size_t hgd_spmm_col_blocks_workspace_size(int64_t n_rows, int32_t n_blocks);
hgd_status hgd_spmm_col_blocks(const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                               int64_t n_cols, int32_t n_blocks, int64_t* blk_start,
                               int32_t* blk_col, int32_t* blk_perm, void* workspace,
                               size_t workspace_bytes, void* stream);
hgd_status hgd_spmm_blocked(const int64_t* blk_start, const int32_t* blk_col,
                            const float* blk_val, const float* row_scale, int64_t n_rows,
                            int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                            const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d,
                            int32_t epilogue, float slope, int32_t n_blocks, void* stream);

/* ------------------------------------------------------------------------------------------
 * hgd_spmm_blocked over tables stored in bfloat16 (x_dtype / y_dtype as hgd_spmm_dt, over the same
 * block-major copy of hgd_spmm_col_blocks). Replaces the same call sites as hgd_spmm
 * (torch.sparse.mm(adj, X), model/graph/HCCF.py:199; torch.sparse.mm(adj.t(), X),
 * model/graph/HGNN_HD4.py:459-462, model/graph/HGCN.py:173-175) when the embedding table is kept
 * or staged in 16 bits AND is too large for the Infinity Cache (a 10 M × 64 bf16 table: 1.28 GB).
 * f32 / f32 codes forward to hgd_spmm_blocked (bitwise its output); n_blocks = 1 is bitwise
 * hgd_spmm_dt without a plan.
 *   fp32 Y: the running partial of a row lives in Y, as in hgd_spmm_blocked; no workspace.
 *   bf16 Y: the partial must not be rounded per block, so it lives in an fp32 scratch in
 *     `workspace`: block 0 writes it, the blocks between add to it, the last block adds it, applies
 *     the activation and stores Y once. A bf16 Y is therefore the fp32 Y of the same call rounded
 *     to nearest even, bit for bit. The scratch is indexed by row as Y is (a row range touches
 *     only its own rows) at the hop's full width: hgd_spmm_blocked_dt_workspace_size is
 *     n_rows·d·4 bytes rounded up to 256 (0 for an fp32 Y and for n_blocks <= 1). The full width,
 *     not one column pass's: the pass width follows the alignment of the call's pointers and the
 *     tuning, which a size query does not see. The 16-byte path also needs the workspace 16-byte
 *     aligned. Too small a workspace: HGD_ERR_WORKSPACE.
 * The call allocates nothing and does not synchronise (graph-capturable). HGD_TUNE_SPMM_BLOCKED_SEG
 * has no effect on a 16-bit hop.
 *
 * hgd_spmm_blocks_for_dt: the size rule by the table's element type. HGD_DT_F32 answers as
 * hgd_spmm_blocks_for; a 16-bit table answers 0: measured on MI355X, no block
 * count from 2 to 8 beat the plain bf16 hop over a 1.28, 2.56 or 5.12 GB table.
 * ---------------------------------------------------------------------------------------- */
size_t hgd_spmm_blocked_dt_workspace_size(int64_t n_rows, int32_t d, int32_t y_dtype,
                                          int32_t n_blocks);
hgd_status hgd_spmm_blocked_dt(const int64_t* blk_start, const int32_t* blk_col,
                               const float* blk_val, const float* row_scale, int64_t n_rows,
                               int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                               const void* X, int32_t x_dtype, int64_t ldx, void* Y,
                               int32_t y_dtype, int64_t ldy, int32_t d, int32_t epilogue,
                               float slope, int32_t n_blocks, void* workspace,
                               size_t workspace_bytes, void* stream);
int32_t hgd_spmm_blocks_for_dt(int64_t n_src_rows, int32_t d, int32_t x_dtype);

/* ------------------------------------------------------------------------------------------
 * The same hop (hgd_spmm, every row, fp32) with the rows WALKED in ascending order of their
 * smallest column, so that rows sharing a source row run next to each other and find it in L2.
 * Replaces the same call sites as hgd_spmm (torch.sparse.mm(adj, X), model/graph/HCCF.py:199).
 * Nothing inside a row changes — the same fmaf chain in edge order — so Y is bitwise hgd_spmm's.
 *
 * hgd_spmm_row_order builds the order of a structure (its rows' columns in any order), once:
 *   order:    int32 [n_rows], the row processed at position p; ascending smallest column (an
 *             empty row counts as n_cols), ties in natural row order (hgd_sort_perm, stable)
 *   rowptr_o: int64 [n_rows+1], the row pointers in processing order
 *   col_o:    int32 [nnz], the columns of the rows in that order, each row's in its own order
 *   perm:     int32 [nnz], the source position of every entry — gather per-nonzero weights
 *             through it and per-row scales through `order` (hgd_gather32); nnz < 2^31
 * No atomics, stream-ordered, no host synchronisation. Workspace:
 * hgd_spmm_row_order_workspace_size.
 *
 * hgd_spmm_ordered: hgd_spmm's arguments with rowptr / col / val / row_scale the ORDERED copies
 * and out_row = order: position p writes Y row out_row[p]. HGD_ERR_UNSUPPORTED for a plan with
 * split rows or HGD_PLAN_SEGMENTED and for a row range other than [0, n_rows) (and, inside the
 * library, with source blocks that bring no orders of their own). With a mask, a fused row
 * epilogue or a 16-bit side: the ordered twins further down (hgd_spmm_fused_ordered, ...).
 * ---------------------------------------------------------------------------------------- */
/* The size rule both hosts use: 1 when a hop of nnz nonzeros over n_rows rows
 * gathering n_src_rows rows at width d should run ordered, else 0. */
int32_t hgd_spmm_row_order_for(int64_t n_rows, int64_t n_src_rows, int64_t nnz, int32_t d);
size_t hgd_spmm_row_order_workspace_size(int64_t n_rows);
hgd_status hgd_spmm_row_order(const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                              int64_t n_cols, int32_t* order, int64_t* rowptr_o, int32_t* col_o,
                              int32_t* perm, void* workspace, size_t workspace_bytes,
                              void* stream);
hgd_status hgd_spmm_ordered(const int64_t* rowptr, const int32_t* col, const float* val,
                            const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                            int64_t row_begin, int64_t row_end, const float* X, int64_t ldx,
                            float* Y, int64_t ldy, int32_t d, int32_t epilogue, float slope,
                            const hgd_split_plan* plan, void* workspace, size_t workspace_bytes,
                            const int32_t* out_row, void* stream);

/* ------------------------------------------------------------------------------------------
 * hgd_spmm_blocked (every row, fp32) with the rows of EACH SOURCE BLOCK walked in ascending order
 * of the first (smallest) column they have in that block: the two ideas above together, so that
 * the first gather of most row pieces of a pass is an L2 hit. Replaces the same call sites as
 * hgd_spmm_blocked (torch.sparse.mm(adj.t(), X), model/graph/HGNN_HD4.py:459-462). Each piece is
 * the same fmaf chain in edge order and block k's partial is added to Y in the same block order,
 * so Y is bitwise hgd_spmm_blocked's.
 *
 * hgd_spmm_col_blocks_ordered builds what hgd_spmm_col_blocks builds with block k's pieces laid
 * out in that order (a row without a nonzero in block k counts as n_cols and sorts last; ties in
 * natural row order, hgd_sort_perm is stable):
 *   blk_start:   int64 [n_blocks·n_rows + 1], the piece at POSITION p of block k is
 *                [blk_start[k·n_rows + p], blk_start[k·n_rows + p + 1]) of blk_col; closed by nnz
 *   blk_out_row: int32 [n_blocks·n_rows], the row position p of block k holds — gather per-row
 *                scales through it (hgd_gather32) to get hgd_spmm_blocked_ordered's blk_row_scale
 *   blk_col, blk_perm (may be NULL): as hgd_spmm_col_blocks'; a piece's columns keep their order
 * blk_col doubles as the builder's scratch. No atomics, stream-ordered, no host synchronisation.
 * Workspace: hgd_spmm_col_blocks_ordered_workspace_size.
 *
 * hgd_spmm_blocked_ordered: blk_row_scale is [n_blocks·n_rows] in processing order, or NULL.
 * Inside the library a mask, a fused row epilogue, a split plan and a row range stay refused
 * (HGD_ERR_UNSUPPORTED); the entry point takes none of them.
 * ---------------------------------------------------------------------------------------- */
/* The size rule both hosts use: 1 when a hop of nnz nonzeros over n_rows rows
 * gathering n_src_rows rows at width d in n_blocks source blocks should order each block. */
int32_t hgd_spmm_block_order_for(int64_t n_rows, int64_t n_src_rows, int64_t nnz, int32_t d,
                                 int32_t n_blocks);
size_t hgd_spmm_col_blocks_ordered_workspace_size(int64_t n_rows, int32_t n_blocks);
hgd_status hgd_spmm_col_blocks_ordered(const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                                       int64_t n_cols, int32_t n_blocks, int64_t* blk_start,
                                       int32_t* blk_col, int32_t* blk_perm, int32_t* blk_out_row,
                                       void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_spmm_blocked_ordered(const int64_t* blk_start, const int32_t* blk_col,
                                    const float* blk_val, const float* blk_row_scale,
                                    const int32_t* blk_out_row, int64_t n_rows,
                                    int64_t n_src_rows, const float* X, int64_t ldx, float* Y,
                                    int64_t ldy, int32_t d, int32_t epilogue, float slope,
                                    int32_t n_blocks, void* stream);

/* ------------------------------------------------------------------------------------------
 * The two ordered hops above over ANY row order, and the GREEDY SHARED-COLUMN order they are built
 * for: the next row walked is one that shares the most columns with what its XCD's L2 still holds
 * (modelled 20–23 % of a short-row hop's gathers hit L2 against 10 % in min-column
 * order). The kernels take any order, so Y stays bitwise hgd_spmm's / hgd_spmm_blocked's.
 *
 * hgd_row_order_greedy builds the order on the HOST, over host pointers, without a HIP call (the
 * structure does not change from call to call: once per structure). The rows are cut into n_xcd
 * natural ranges ("parts"), sized to what each XCD's workgroups hold when workgroup w — positions
 * [w·rows_per_wg, (w+1)·rows_per_wg), only the last one short — runs on XCD w mod n_xcd; each part
 * is cut evenly into chunks_per_xcd chunks, every chunk is walked greedily on its own, and
 * position (n_xcd·s + x)·rows_per_wg + j takes element s·rows_per_wg + j of part x, so XCD x walks
 * part x from its start to its end. Empty rows come last, in natural order, after the placed ones.
 *   window:  the gathers an XCD's L2 remembers (hgd_spmm_order_geometry)
 *   col_cap: a column with more entries in a chunk moves no row (it is in L2 anyway); bounds the
 *            build at 2·nnz·min(column degree, col_cap) list moves. HGD_ORDER_COL_CAP = 1024
 *   threads: the chunks run on up to that many std::threads; 0 = min(chunks, OMP_NUM_THREADS if
 *            set, else 8). The order depends on the other arguments only, never on this one.
 * hgd_col_block_order_greedy does the same for every source block of a structure whose rows'
 * columns ascend (hgd_spmm_col_blocks' cuts ⌊n_cols·k / n_blocks⌋): blk_order_out
 * [n_blocks·n_rows], block k's order at k·n_rows, the rows without a nonzero in the block last.
 * HGD_ERR_INVALID_ARG for a column outside [0, n_cols) (or columns that do not ascend),
 * HGD_ERR_WORKSPACE when the host has no memory for a chunk's tables; no exception leaves either.
 *
 * hgd_row_order_greedy_pooled / hgd_col_block_order_greedy_pooled: the same layout (the parts'
 * sizes, the interleave, the empty rows last) with one chunk per part, but the XCDs of a group of
 * xcds_per_pool (which must divide n_xcd) take their rows in turn from ONE pool, the natural range
 * their parts cover together: in round s walker 0, 1, ... each take their s-th row, every walker
 * with its own window and its own counts over the whole pool, so each chooses among xcds_per_pool
 * times as many rows (modelled: 27 % of the gathers into users hit with one pool of 8, 22 % with 8
 * parts walked alone). xcds_per_pool = 1 is hgd_row_order_greedy(chunks_per_xcd = 1), bit for bit.
 * The block form makes every source block a pool of its own kind. A pool is walked by a team of
 * threads over a number of row ranges fixed by the arguments: the order still never depends on
 * `threads` (0 = min(work, OMP_NUM_THREADS if set, else 8)). Host memory: about 10 bytes per row
 * and walker of a pool and 4 per entry, beside the structure.
 *
 * hgd_spmm_row_order_from / hgd_spmm_col_blocks_ordered_from are hgd_spmm_row_order /
 * hgd_spmm_col_blocks_ordered after their sorts, over the caller's DEVICE order (blk_order doubles
 * as the blk_out_row of the hop): the same outputs for the same order, bit for bit. Both first
 * check on the device that the order is a permutation (of every block) — a flag array and one
 * reduction, no atomics — and WAIT FOR THE STREAM to read the answer (the caller copied the
 * structure to the host to build the order: it has synchronised already; never inside a capture):
 * HGD_ERR_INVALID_ARG otherwise, before anything is read through the order.
 *
 * hgd_spmm_order_geometry: the rows per workgroup and the window of the fp32 hop at width d
 * (blocked: the source-blocked hop), from the launcher's own pass plan over 16-byte aligned rows;
 * window = 4 MiB / the bytes of a source row one pass gathers. Returns 0 for a bad argument.
 * hgd_spmm_row_order_kind_for: the rule both hosts use, HGD_ORDER_* for a hop in n_blocks source
 * blocks (<= 1: not blocked): HGD_ORDER_GREEDY wherever hgd_spmm_row_order_for /
 * hgd_spmm_block_order_for order the hop, else HGD_ORDER_NONE.
 * ---------------------------------------------------------------------------------------- */
#define HGD_ORDER_NONE 0
#define HGD_ORDER_MIN_COLUMN 1
#define HGD_ORDER_GREEDY 2
#define HGD_ORDER_COL_CAP 1024
hgd_status hgd_row_order_greedy(const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                                int64_t n_cols, int64_t window, int32_t col_cap,
                                int32_t rows_per_wg, int32_t n_xcd, int32_t chunks_per_xcd,
                                int32_t threads, int32_t* order_out);
hgd_status hgd_col_block_order_greedy(const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                                      int64_t n_cols, int32_t n_blocks, int64_t window,
                                      int32_t col_cap, int32_t rows_per_wg, int32_t n_xcd,
                                      int32_t chunks_per_xcd, int32_t threads,
                                      int32_t* blk_order_out);
hgd_status hgd_row_order_greedy_pooled(const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                                       int64_t n_cols, int64_t window, int32_t col_cap,
                                       int32_t rows_per_wg, int32_t n_xcd, int32_t xcds_per_pool,
                                       int32_t threads, int32_t* order_out);
hgd_status hgd_col_block_order_greedy_pooled(const int64_t* rowptr, const int32_t* col,
                                             int64_t n_rows, int64_t n_cols, int32_t n_blocks,
                                             int64_t window, int32_t col_cap, int32_t rows_per_wg,
                                             int32_t n_xcd, int32_t xcds_per_pool,
                                             int32_t threads, int32_t* blk_order_out);
size_t hgd_spmm_row_order_from_workspace_size(int64_t n_rows);
hgd_status hgd_spmm_row_order_from(const int32_t* order, const int64_t* rowptr, const int32_t* col,
                                   int64_t n_rows, int64_t n_cols, int64_t* rowptr_o,
                                   int32_t* col_o, int32_t* perm, void* workspace,
                                   size_t workspace_bytes, void* stream);
size_t hgd_spmm_col_blocks_ordered_from_workspace_size(int64_t n_rows, int32_t n_blocks);
hgd_status hgd_spmm_col_blocks_ordered_from(const int32_t* blk_order, const int64_t* rowptr,
                                            const int32_t* col, int64_t n_rows, int64_t n_cols,
                                            int32_t n_blocks, int64_t* blk_start, int32_t* blk_col,
                                            int32_t* blk_perm, void* workspace,
                                            size_t workspace_bytes, void* stream);
int32_t hgd_spmm_order_geometry(int32_t d, int32_t blocked, int32_t* rows_per_wg, int64_t* window);
int32_t hgd_spmm_row_order_kind_for(int64_t n_rows, int64_t n_src_rows, int64_t nnz, int32_t d,
                                    int32_t n_blocks);

/* ------------------------------------------------------------------------------------------
 * hgd_spmm_blocked_ordered WITHOUT THE WEIGHT STREAM, for weights that are a per-source-row scale
 * expanded over the nonzeros (val[e] = S[col[e]], the degree scales of a binary incidence:
 * torch.sparse.mm(adj.t(), X) with adj = D^-1/2 H ..., model/graph/HGNN_HD4.py:459-462): S has few
 * distinct values, so a nonzero is ONE 32-bit word
 *   ent = (col − base_k) | code << idx_bits
 * with base_k = ⌊n_src_rows·k / n_blocks⌋ the first source row of its block k (hgd_spmm_col_blocks'
 * cuts) and dict[code] the weight. The hop reads 4 bytes per nonzero instead of 8; each piece is
 * the same fmaf chain over the same weights, so Y is bitwise hgd_spmm_blocked_ordered's with
 * blk_val[e] = dict[code of e].
 *
 * idx_bits is 1..31 (22 by default: a block of at most 4 Mi source rows beside a 10-bit code);
 * every block must have at most 2^idx_bits source rows and the dictionary 1..min(2^(32−idx_bits),
 * HGD_SPMM_PACKED_MAX_DICT) entries (it lives in 4 KB of LDS), else HGD_ERR_UNSUPPORTED.
 *
 * hgd_spmm_pack_entries builds ent [nnz] (uint32) from blk_start / blk_col of
 * hgd_spmm_col_blocks_ordered (or hgd_spmm_col_blocks) and src_code [n_src_rows] (int32, every
 * code < n_dict: trusted as the columns are), one thread per nonzero, which finds its block from
 * the n_blocks + 1 block boundaries blk_start[k·n_rows]. No atomics, no workspace, stream-ordered,
 * no host synchronisation. nnz is the caller's (blk_start[n_blocks·n_rows]).
 *
 * hgd_spmm_blocked_packed: hgd_spmm_blocked_ordered's arguments with ent in place of blk_col /
 * blk_val, plus the dictionary. Refuses what hgd_spmm_blocked_ordered refuses.
 * ---------------------------------------------------------------------------------------- */
#define HGD_SPMM_PACKED_MAX_DICT 1024
#define HGD_SPMM_PACKED_IDX_BITS 22
/* hgd_spmm_packed_fits: 1 when the format can hold the hop (n_blocks in 1..64, every block within
 * 2^idx_bits source rows, 1 <= n_dict <= min(2^(32−idx_bits), HGD_SPMM_PACKED_MAX_DICT)): what the
 * builder and the hop accept.
 * hgd_spmm_packed_for: the rule both hosts use: 1 when a block-ordered hop
 * gathering n_src_rows rows in n_blocks >= 2 source blocks whose weights have n_dict distinct values
 * should run packed at idx_bits — it fits, and a block has at least 65,536 source rows (the
 * smallest slice hgd_spmm_block_order_for orders: below it the blocks were forced). */
int32_t hgd_spmm_packed_fits(int64_t n_src_rows, int32_t n_blocks, int64_t n_dict,
                             int32_t idx_bits);
int32_t hgd_spmm_packed_for(int64_t n_src_rows, int32_t n_blocks, int64_t n_dict,
                            int32_t idx_bits);
hgd_status hgd_spmm_pack_entries(const int64_t* blk_start, const int32_t* blk_col,
                                 const int32_t* src_code, int64_t n_rows, int64_t n_src_rows,
                                 int64_t nnz, int32_t n_blocks, int32_t n_dict, int32_t idx_bits,
                                 uint32_t* ent, void* stream);
hgd_status hgd_spmm_blocked_packed(const int64_t* blk_start, const uint32_t* ent,
                                   const float* dict, int32_t n_dict, int32_t idx_bits,
                                   const float* blk_row_scale, const int32_t* blk_out_row,
                                   int64_t n_rows, int64_t n_src_rows, const float* X, int64_t ldx,
                                   float* Y, int64_t ldy, int32_t d, int32_t epilogue, float slope,
                                   int32_t n_blocks, void* stream);

/* ------------------------------------------------------------------------------------------
 * hgd_spmm_blocked (fp32 in and out, a row range honoured) over a structure WITH SPLIT ROWS: the
 * skewed catalogues hgd_spmm_blocked leaves to hgd_spmm. Replaces the same call sites as
 * hgd_spmm_blocked (torch.sparse.mm(adj.t(), X), model/graph/HGNN_HD4.py:459-462,
 * model/graph/HCCF.py:199) when the gathered table is too large for the Infinity Cache and some
 * rows are long enough to be split.
 *   blk_start / blk_col / blk_val: the block-major copy of hgd_spmm_col_blocks.
 *   plans: a HOST array of n_blocks split plans; plan k is the plan of block k's own CSR, built
 *     with hgd_split_plan_count / hgd_split_plan_build on blk_start + k·n_rows over n_rows rows
 *     with the parent's threshold and chunk. A row is therefore heavy PER BLOCK: a row of 5,000
 *     nonzeros over 4 blocks may be light in all of them. A plan with n_heavy == 0 (or
 *     threshold <= 0) is an empty plan; HGD_PLAN_SEGMENTED in any plan is HGD_ERR_UNSUPPORTED.
 *   workspace: hgd_spmm_blocked_split_workspace_size(plans, n_blocks, d) bytes, the maximum over
 *     the blocks of hgd_spmm_workspace_size(plan k, d): the blocks run in stream order and reuse
 *     it. Too small: HGD_ERR_WORKSPACE.
 * Per column pass (at most 128 columns, as hgd_spmm_blocked) and for k = 0 … n_blocks−1: one
 * launch for block k's chunks and its light rows, one for the fix-up of its heavy rows. Block
 * k > 0 adds to Y, the activation runs after the last block, and Y is written exactly once per
 * row and block, whether that block's piece of the row is heavy (the fix-up writes it) or light
 * (the row kernel does). Every sum is in a fixed order, no atomics: two runs are bitwise equal.
 * HGD_TUNE_SPMM_BLOCKED_SEG applies to the blocks without heavy rows only.
 * With every plan empty the call is bitwise hgd_spmm_blocked; with n_blocks = 1 it is bitwise
 * hgd_spmm with that plan (and runs in hgd_spmm's column passes).
 * The call allocates nothing and does not synchronise (graph-capturable).
 *
 * hgd_spmm_blocks_split_for: the rule both hosts would use for such a structure (host-only):
 * the block count for a hop gathering n_src_rows rows at width d whose plan puts
 * n_chunks·chunk / nnz of the nonzeros in split rows; 0 = run hgd_spmm. Measured on MI355X at
 * 10 M × 1 M × 100 M (profiles/blocked_split/): 4 for a pass's gathered table
 * (n_src_rows × min(d, 128) × 4 bytes) from 2.56 GB to below 5.12 GB with at most 28.62 % of the
 * nonzeros in split rows, where P = 4 beat the plain split hop by 2.5 % on both repeats; 0
 * everywhere else (items ∝ rank^-1 and d = 128 stayed inside the rounds' range).
 * ---------------------------------------------------------------------------------------- */
size_t hgd_spmm_blocked_split_workspace_size(const hgd_split_plan* plans, int32_t n_blocks,
                                             int32_t d);
hgd_status hgd_spmm_blocked_split(const int64_t* blk_start, const int32_t* blk_col,
                                  const float* blk_val, const float* row_scale, int64_t n_rows,
                                  int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                                  const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d,
                                  int32_t epilogue, float slope, int32_t n_blocks,
                                  const hgd_split_plan* plans, void* workspace,
                                  size_t workspace_bytes, void* stream);
int32_t hgd_spmm_blocks_split_for(int64_t n_src_rows, int32_t d, int64_t nnz, int64_t n_chunks,
                                  int32_t chunk);

/* The same hop over the EDGE-DROPPED matrix of SpAdjDropEdge (model/graph/HCCF.py:213-226:
 * mask = floor(rand + keepRate), idxs[:, mask], vals[mask] / keepRate) without building it: the
 * structure is the parent's, `mask` (uint8, this orientation's edge order; for the CSC of the
 * parent that is mask_csr[perm_t]) selects the kept edges, each weighted by val[e] / keep (IEEE
 * fp32 division, as the dropped COO's values; val == NULL keeps all-ones weights, like
 * hgd_dropedge_structure). Kept edges are summed in edge order, so a row's sum equals the hop
 * over the compacted matrix of hgd_dropedge_structure whenever the split plan covers the same
 * rows (no split rows: bit-identical). Replaces the per-step compaction (count, scan, compact,
 * row pointers for the CSR and the CSC) of a training step's drop-edge. */
hgd_status hgd_spmm_masked(const int64_t* rowptr, const int32_t* col, const float* val,
                           const uint8_t* mask, float keep, const float* row_scale,
                           int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                           int64_t row_end, const float* X, int64_t ldx, float* Y, int64_t ldy,
                           int32_t d, int32_t epilogue, float slope, const hgd_split_plan* plan,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused row epilogue of an ED-HNN / HGCN layer. Replaces the torch ops
 * the reference runs on the hop output, each an extra [N,d] HBM round trip and launch:
 *   LayerNorm + residual     Xe = LN0(HGCNConv(adj, Xve)) + Xve   model/layers/EquivSetConv.py:86-107,
 *                                                                 model/graph/HGNN_HD3.py:705-720
 *   restart blend            X = (1-α)·Xv + α·X0                   model/layers/layers2/EquivSetConv2.py:96
 * For every row r written by the hop (z = row_scale[r]·Σ of hgd_spmm):
 *   a = act(z)                         (act_out[r] = a when act_out != NULL)
 *   b = layer_norm ? (a - μ_r)·rstd_r·γ + β : a      (biased variance, rstd = 1/sqrt(var+eps);
 *                                                      stats[2r] = μ_r, stats[2r+1] = rstd_r)
 *   Y[r] = out_scale·b + res1_scale·res1[r] + res2_scale·res2[r]    (NULL residuals skipped)
 *   sum_out[r] = Y[r] + sum_res[r]                                    (when sum_out != NULL)
 * layer_norm needs the whole row in one lane group: d <= 256 with 16-byte aligned rows (X, Y,
 * residuals, act_out, leading dims % 4 == 0), or d <= 64 otherwise (HGD_ERR_UNSUPPORTED beyond).
 * act must be NONE or have slope >= 0, so that act'(z) can be read from the sign of a.
 * ---------------------------------------------------------------------------------------- */
typedef struct hgd_row_epilogue {
  int32_t act;            /* hgd_epilogue */
  float slope;
  int32_t layer_norm;     /* 0 / 1 */
  float ln_eps;
  const float* ln_gamma;  /* [d] or NULL (= 1) */
  const float* ln_beta;   /* [d] or NULL (= 0) */
  float out_scale;
  const float* res1;      /* [n_rows, ld_res1] or NULL */
  int64_t ld_res1;
  float res1_scale;
  const float* res2;
  int64_t ld_res2;
  float res2_scale;
  float* act_out;         /* [n_rows, ld_act] or NULL */
  int64_t ld_act;
  float* stats;           /* [n_rows, 2] or NULL */
  /* optional second output after the residuals: sum_out[r] = Y[r] + sum_res[r] (HCCF's
   * backward: the layer gradient dh and dh + the InfoNCE gradient of the layer below in one
   * store); both NULL or both set. res1 / res2 may alias Y (each row is read before it is
   * written, by the same lanes). */
  const float* sum_res;
  int64_t ld_sum_res;
  float* sum_out;
  int64_t ld_sum_out;
} hgd_row_epilogue;

/* hgd_spmm with the fused row epilogue `epi` (which replaces hgd_spmm's epilogue/slope). */
hgd_status hgd_spmm_fused(const int64_t* rowptr, const int32_t* col, const float* val,
                          const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                          int64_t row_begin, int64_t row_end, const float* X, int64_t ldx,
                          float* Y, int64_t ldy, int32_t d, const hgd_row_epilogue* epi,
                          const hgd_split_plan* plan, void* workspace, size_t workspace_bytes,
                          void* stream);

/* hgd_spmm_masked (the edge-dropped view) with the fused row epilogue `epi`. HCCF's layer
 * (model/graph/HCCF.py:182-187): gcn = A_drop·h stored through act_out while the row store adds
 * the layer's hypergraph term as res1, so hidden[k+1] = gcn + hgnn needs no separate add; the
 * backward hop adds the layer-sum gradient the same way. */
hgd_status hgd_spmm_masked_fused(const int64_t* rowptr, const int32_t* col, const float* val,
                                 const uint8_t* mask, float keep, const float* row_scale,
                                 int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                 int64_t row_end, const float* X, int64_t ldx, float* Y,
                                 int64_t ldy, int32_t d, const hgd_row_epilogue* epi,
                                 const hgd_split_plan* plan, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* hgd_spmm_fused / hgd_spmm_masked_fused gathering from a table stored in bfloat16 (x_dtype, ldx as
 * hgd_spmm_dt). They replace the call sites those two replace (LN0(HGCNConv(adj, Xve)) + Xve,
 * model/layers/EquivSetConv.py:86-107, model/graph/HGNN_HD3.py:705-720; the restart blend,
 * model/layers/layers2/EquivSetConv2.py:96; HCCF's layer, model/graph/HCCF.py:182-187) when the hop
 * input is kept or staged in 16 bits: the gathered rows are nnz·2d bytes instead of nnz·4d.
 * Only the gathered table is 16-bit. Y is fp32, and so are the residuals, act_out, the LayerNorm
 * statistics, γ, β, sum_res / sum_out and the split-row partials; a bf16 element is widened
 * exactly and the sum is hgd_spmm's fp32 fmaf chain in edge order.
 *   y16 (bf16 [n_rows, ld_y16], or NULL): a second output, the row just written to Y rounded to
 *   nearest even from the same registers — the table the next layer's first hop gathers, without a
 *   cast pass over Y. ld_y16 >= d; it takes part in the 16-byte test like the side tables
 *   (ld_y16 % 8 == 0), and the 16-byte path needs d % 8 == 0.
 *   x_dtype == HGD_DT_F32 with y16 == NULL forwards to hgd_spmm_fused / hgd_spmm_masked_fused
 *   (bitwise theirs); HGD_DT_F32 with a y16 is HGD_ERR_UNSUPPORTED.
 * layer_norm needs d <= 256 on the 16-byte path (a group of d/8 lanes holds the row), d <= 64
 * otherwise. Workspace: hgd_spmm_workspace_size, unchanged. A plan with HGD_PLAN_SEGMENTED is
 * walked by the row kernel (the same sums). */
hgd_status hgd_spmm_fused_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                             const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                             int64_t row_begin, int64_t row_end, const void* X, int32_t x_dtype,
                             int64_t ldx, float* Y, int64_t ldy, int32_t d,
                             const hgd_row_epilogue* epi, void* y16, int64_t ld_y16,
                             const hgd_split_plan* plan, void* workspace, size_t workspace_bytes,
                             void* stream);
hgd_status hgd_spmm_masked_fused_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                                    const uint8_t* mask, float keep, const float* row_scale,
                                    int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                    int64_t row_end, const void* X, int32_t x_dtype, int64_t ldx,
                                    float* Y, int64_t ldy, int32_t d,
                                    const hgd_row_epilogue* epi, void* y16, int64_t ld_y16,
                                    const hgd_split_plan* plan, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The ORDERED TWINS of the fused, masked and 16-bit hops: hgd_spmm_ordered's row walk (any order:
 * hgd_spmm_row_order's, the greedy one through hgd_spmm_row_order_from) for every hop a model
 * issues. Each takes its twin's arguments plus out_row before stream, where hgd_spmm_ordered has
 * it, and replaces the call site its twin replaces when the structure's rows are walked in an
 * order:
 *   hgd_spmm_fused_ordered            hgd_spmm_fused            LN0(HGCNConv(adj, Xve)) + Xve,
 *                                     model/layers/EquivSetConv.py:86-107, model/graph/HGNN_HD3.py:705-720
 *   hgd_spmm_masked_ordered           hgd_spmm_masked           SpAdjDropEdge + torch.sparse.mm,
 *                                     model/graph/HCCF.py:213-226, :199
 *   hgd_spmm_masked_fused_ordered     hgd_spmm_masked_fused     HCCF's layer, model/graph/HCCF.py:182-187
 *   hgd_spmm_ordered_dt               hgd_spmm_dt               torch.sparse.mm(adj, X) over a 16-bit
 *   hgd_spmm_masked_ordered_dt        hgd_spmm_masked_dt        table or output, model/graph/HCCF.py:199
 *   hgd_spmm_fused_ordered_dt         hgd_spmm_fused_dt         the fused layers above over a
 *   hgd_spmm_masked_fused_ordered_dt  hgd_spmm_masked_fused_dt  bfloat16 table
 * The ordered copies, indexed by POSITION p (as for hgd_spmm_ordered):
 *   rowptr, col, val: hgd_spmm_row_order's rowptr_o / col_o and the weights gathered through perm;
 *   row_scale: the per-row scales gathered through the order (hgd_gather32);
 *   mask: uint8 [nnz] in the ORDERED ENTRY ORDER — this orientation's mask gathered through the
 *   order's perm (hgd_gather_u8), entry e of the ordered copy beside col[e] and val[e].
 * Indexed by Y ROW (position p writes row out_row[p] of each): Y, and everything epi points to —
 * res1, res2, act_out, stats, sum_res, sum_out — and y16: the caller passes the arrays it passes
 * to the unordered twin, unchanged. ln_gamma / ln_beta are per column.
 * Nothing inside a row changes — the same fmaf chain over the (kept) entries in edge order, the
 * row epilogue in the same registers — so every output is BITWISE the unordered twin's.
 * HGD_ERR_UNSUPPORTED, before any launch: a plan with split rows or HGD_PLAN_SEGMENTED, a row range
 * other than [0, n_rows), and a LayerNorm row that does not fit one column pass (as the twin).
 * HGD_ERR_INVALID_ARG for a null out_row (n_rows > 0). The _dt twins forward f32 → f32 to the fp32
 * ordered twins, as the unordered ones forward to theirs. Only U = 8 with the default cache policy
 * is instantiated for these forms, as for their twins.
 *
 * hgd_spmm_order_geometry_dt / hgd_spmm_row_order_for_dt: hgd_spmm_order_geometry and
 * hgd_spmm_row_order_for for the form that will run — x_dtype / y_dtype (HGD_DT_*), fused (with a
 * row epilogue), masked. The geometry is the launcher's own pass plan of that form: a 16-bit side
 * has 8-column lanes and 128-column passes, the window counts pieces of min(d, pass) elements of
 * X, and a fused row is one pass of up to 256 columns (fp32: 64 lanes, 4 rows per workgroup at
 * d = 256). 0 for an unknown dtype code, a fused hop into a 16-bit Y or over source blocks. The
 * plain fp32 form answers as the queries above. The rule of every other form is set by
 * measurement: 0 wherever the ordered twin did not beat the unordered call.
 * ---------------------------------------------------------------------------------------- */
hgd_status hgd_spmm_fused_ordered(const int64_t* rowptr, const int32_t* col, const float* val,
                                  const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                                  int64_t row_begin, int64_t row_end, const float* X, int64_t ldx,
                                  float* Y, int64_t ldy, int32_t d, const hgd_row_epilogue* epi,
                                  const hgd_split_plan* plan, void* workspace,
                                  size_t workspace_bytes, const int32_t* out_row, void* stream);
hgd_status hgd_spmm_masked_ordered(const int64_t* rowptr, const int32_t* col, const float* val,
                                   const uint8_t* mask, float keep, const float* row_scale,
                                   int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                   int64_t row_end, const float* X, int64_t ldx, float* Y,
                                   int64_t ldy, int32_t d, int32_t epilogue, float slope,
                                   const hgd_split_plan* plan, void* workspace,
                                   size_t workspace_bytes, const int32_t* out_row, void* stream);
hgd_status hgd_spmm_masked_fused_ordered(const int64_t* rowptr, const int32_t* col,
                                         const float* val, const uint8_t* mask, float keep,
                                         const float* row_scale, int64_t n_rows,
                                         int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                                         const float* X, int64_t ldx, float* Y, int64_t ldy,
                                         int32_t d, const hgd_row_epilogue* epi,
                                         const hgd_split_plan* plan, void* workspace,
                                         size_t workspace_bytes, const int32_t* out_row,
                                         void* stream);
hgd_status hgd_spmm_ordered_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                               const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                               int64_t row_begin, int64_t row_end, const void* X, int32_t x_dtype,
                               int64_t ldx, void* Y, int32_t y_dtype, int64_t ldy, int32_t d,
                               int32_t epilogue, float slope, const hgd_split_plan* plan,
                               void* workspace, size_t workspace_bytes, const int32_t* out_row,
                               void* stream);
hgd_status hgd_spmm_masked_ordered_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                                      const uint8_t* mask, float keep, const float* row_scale,
                                      int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                      int64_t row_end, const void* X, int32_t x_dtype, int64_t ldx,
                                      void* Y, int32_t y_dtype, int64_t ldy, int32_t d,
                                      int32_t epilogue, float slope, const hgd_split_plan* plan,
                                      void* workspace, size_t workspace_bytes,
                                      const int32_t* out_row, void* stream);
hgd_status hgd_spmm_fused_ordered_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                                     const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                                     int64_t row_begin, int64_t row_end, const void* X,
                                     int32_t x_dtype, int64_t ldx, float* Y, int64_t ldy,
                                     int32_t d, const hgd_row_epilogue* epi, void* y16,
                                     int64_t ld_y16, const hgd_split_plan* plan, void* workspace,
                                     size_t workspace_bytes, const int32_t* out_row, void* stream);
hgd_status hgd_spmm_masked_fused_ordered_dt(const int64_t* rowptr, const int32_t* col,
                                            const float* val, const uint8_t* mask, float keep,
                                            const float* row_scale, int64_t n_rows,
                                            int64_t n_src_rows, int64_t row_begin,
                                            int64_t row_end, const void* X, int32_t x_dtype,
                                            int64_t ldx, float* Y, int64_t ldy, int32_t d,
                                            const hgd_row_epilogue* epi, void* y16,
                                            int64_t ld_y16, const hgd_split_plan* plan,
                                            void* workspace, size_t workspace_bytes,
                                            const int32_t* out_row, void* stream);
int32_t hgd_spmm_order_geometry_dt(int32_t d, int32_t blocked, int32_t x_dtype, int32_t y_dtype,
                                   int32_t fused, int32_t* rows_per_wg, int64_t* window);
int32_t hgd_spmm_row_order_for_dt(int64_t n_rows, int64_t n_src_rows, int64_t nnz, int32_t d,
                                  int32_t x_dtype, int32_t y_dtype, int32_t fused,
                                  int32_t masked);

/* The same row epilogue applied to an existing matrix Z [n_rows, ldz] (z = Z[r], no hop): the
 * LayerNorms that do not follow a hop, e.g. the MLP InputNorm of model/layers/MLP.py:65-71,109-110.
 * Needs d <= 256 with 16-byte aligned rows, or d <= 64. Y may alias Z. */
hgd_status hgd_row_epilogue_forward(const float* Z, int64_t ldz, int64_t n_rows, int32_t d,
                                    const hgd_row_epilogue* epi, float* Y, int64_t ldy,
                                    void* stream);

/* Backward of the row epilogue up to z (the residual gradients are res_scale·dY, left to the
 * caller): dZ = act'(a) ⊙ LN_bwd(out_scale·dY), with LN_bwd the LayerNorm input gradient
 * rstd·(ĝ - mean(ĝ) - â·mean(ĝ⊙â)), ĝ = γ⊙dy, â = (a-μ)·rstd recomputed from act_out and stats.
 * dgamma = Σ_r dy⊙â, dbeta = Σ_r dy (written, not accumulated; summed in a fixed order, so the
 * result is deterministic). act_out is required when act != NONE or layer_norm. */
size_t hgd_row_epilogue_backward_workspace_size(int64_t n_rows, int32_t d);
hgd_status hgd_row_epilogue_backward(const float* dY, int64_t ldy, const float* act_out,
                                     int64_t ld_act, const float* stats, const float* ln_gamma,
                                     int64_t n_rows, int32_t d, int32_t act, float slope,
                                     int32_t layer_norm, float out_scale, float* dZ, int64_t ldz,
                                     float* dgamma, float* dbeta, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* hgd_row_epilogue_backward with the element type of dZ chosen by the caller (dz_dtype:
 * HGD_DT_F32 or HGD_DT_BF16; ldz counts elements of that type). It serves the call sites
 * hgd_row_epilogue_backward serves (the LayerNorm, add / blend and LeakyReLU backwards of
 * model/layers/EquivSetConv.py:86-107 and of the layers listed at hgd_spmm_fused_dt) when the
 * backward hops gather 16-bit tables: the first of them reads nnz·2d bytes of dZ instead of nnz·4d,
 * and no cast pass runs over the table.
 *   HGD_DT_BF16: the arithmetic is hgd_row_epilogue_backward's, in fp32 throughout; each element
 *   of dZ is rounded to nearest even once, in the store, so dZ is bitwise the bfloat16 cast of the
 *   fp32 entry point's dZ. dgamma / dbeta are summed from the unrounded values and are bitwise the
 *   fp32 entry point's. The 16-byte path (four columns per lane, an 8-byte store of dZ) needs dZ
 *   aligned to 8 bytes and ldz % 4 == 0 next to the fp32 tables' 16-byte test; otherwise a lane
 *   owns one column. layer_norm needs d <= 256 on the 16-byte path, d <= 64 otherwise.
 *   HGD_DT_F32 forwards to hgd_row_epilogue_backward (bitwise its result; its errors carry its
 *   name). Any other code is HGD_ERR_INVALID_ARG.
 * Workspace: hgd_row_epilogue_backward_workspace_size, unchanged. */
hgd_status hgd_row_epilogue_backward_dt(const float* dY, int64_t ldy, const float* act_out,
                                        int64_t ld_act, const float* stats, const float* ln_gamma,
                                        int64_t n_rows, int32_t d, int32_t act, float slope,
                                        int32_t layer_norm, float out_scale, void* dZ,
                                        int32_t dz_dtype, int64_t ldz, float* dgamma,
                                        float* dbeta, void* workspace, size_t workspace_bytes,
                                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Skinny Linear layers on the f32 MFMA: nn.Linear(in, out) over
 * n_rows ≫ in, out — lin_in of model/layers/EquivSetGNN.py:88-89 /
 * layers2/EquivSetGNN2.py:93-94 (with its F.relu) and the MLP layers of
 * model/layers/MLP.py:109-117. W is [out_features, ldw] row-major (nn.Linear.weight); features
 * are multiples of 16, rows 16-byte aligned. Forward: in_features <= 128; backward-data:
 * out_features <= 128. Exact f32 products and sums (order differs from a library GEMM).
 *   forward          Y = relu?(X·Wᵀ + bias)
 *   backward_data    dX = (dY ⊙ [relu_out > 0])·W        (relu_out = the forward Y, or NULL)
 *   backward_weight  dW = (dY ⊙ [relu_out > 0])ᵀ·X, db = Σ_rows dY ⊙ [relu_out > 0]
 *                    (dW written contiguous [out, in]; split-K partials summed in a fixed order)
 * ---------------------------------------------------------------------------------------- */
hgd_status hgd_linear_forward(const float* X, int64_t ldx, int64_t n_rows, int32_t in_features,
                              const float* W, int64_t ldw, int32_t out_features,
                              const float* bias, int32_t relu, float* Y, int64_t ldy,
                              void* stream);
hgd_status hgd_linear_backward_data(const float* dY, int64_t ldy, const float* relu_out,
                                    int64_t ldr, int64_t n_rows, int32_t out_features,
                                    const float* W, int64_t ldw, int32_t in_features, float* dX,
                                    int64_t ldx, void* stream);
size_t hgd_linear_backward_weight_workspace_size(int64_t n_rows, int32_t out_features,
                                                 int32_t in_features);
hgd_status hgd_linear_backward_weight(const float* dY, int64_t ldy, const float* relu_out,
                                      int64_t ldr, const float* X, int64_t ldx, int64_t n_rows,
                                      int32_t out_features, int32_t in_features, float* dW,
                                      float* db, void* workspace, size_t workspace_bytes,
                                      void* stream);

/* Grouped forms of the skinny products above (HCCF's learned hypergraph HCCF.py:201-211 runs
 * every product once for the users and once for the items): one launch for one or two
 * independent products of equal shape class, which is what bounds these ~10 MB products.
 *   hgd_gemm_rows: Y = relu?((A ⊙ [relu_mask > 0])·B + bias) (+ Y when accumulate), A [rows, K]
 *     (16-byte aligned rows), B[k][n] = B[k·bsk + n·bsn]; K a multiple of 16 in [16, 128], N a
 *     multiple of 16; the two products must share K, N, mask presence and the epilogue kind
 *     (plain store, accumulate, or res / Y2; a mixed group is HGD_ERR_INVALID_ARG). The masked
 *     form
 *     (relu_mask set: the backward-data product) takes none of the drop / res / row_inv /
 *     binarize_a epilogues below (HGD_ERR_INVALID_ARG).
 *   hgd_gemm_tn: C [M, N] = (A ⊙ [relu_mask > 0])ᵀ·B over `rows` rows (split-K, partials summed
 *     in slice order: deterministic), colsum_A [M] = Σ_rows A ⊙ mask when non-NULL; the two
 *     products must share M, N and mask presence. Workspace: hgd_gemm_tn_workspace_size. */
typedef struct hgd_gemm_rows_desc {
  const float* A;
  int64_t lda;
  const float* relu_mask; /* [rows, K] or NULL */
  int64_t ldm;
  const float* B;
  int64_t bsk;
  int64_t bsn;
  const float* bias;      /* [N] or NULL */
  int32_t relu;
  int32_t accumulate;
  float* Y;
  int64_t ldy;
  int64_t rows;
  int32_t K;
  int32_t N;
  /* forward epilogue after bias / ReLU (NULL / 0 = off): nn.Dropout — element (row, col) kept as
   * hgd_dropout_apply keeps element row·N + col (rows·N < 2^32) for seed *drop_seed (a device
   * value: a captured step draws it inside the graph), kept values × drop_scale (1 / (1 - p));
   * then the second store Y2 = Y + res (res and Y2 both NULL or both set) — the "+ res" after
   * an ED-HNN block (HGNN_HD4.py:399) */
  const uint64_t* drop_seed;
  float drop_keep;
  float drop_scale;
  const float* res;
  int64_t ldres;
  float* Y2;
  int64_t ldy2;
  /* row_inv (NULL = off): the product's rows scaled by 1 / max(Σ_k A'[r, k], 1) before bias /
   * ReLU and that factor stored to row_inv[r] — with binarize_a, the scatter mean over a vertex's
   * hyperedges of a dense learned hypergraph (EquivSetConv2.py:93 on nonzero(H > 0),
   * EquivSetGNN2.py:105-133); binarize_a: A' = (A > 0 ? 1 : 0) instead of A */
  float* row_inv;
  int32_t binarize_a;
  /* b_row_count (NULL = off): row k of B scaled by 1 / max(b_row_count[k], 1) as it is staged —
   * the hyperedge means D_e^-1·Xe of the mean two-hop from the raw column counts colsum_A of the
   * split-K product that made Xe (same product as scaling B beforehand) */
  const float* b_row_count;
  float b_scale;          /* 0 = off: B × b_scale as it is staged (a Dropout's 1/(1-p) in dX) */
  /* a_drop_seed (NULL = off): nn.Dropout on A as it is loaded — element (row, k) kept as
   * hgd_dropout_apply keeps element row·K + k (rows·K < 2^32) for seed *a_drop_seed, kept values
   * × a_drop_scale, before relu_mask / binarize_a: the ED-HNN block's input dropout inside
   * lin_in (EquivSetGNN2.py:91-92). With relu_mask set, drop_seed is the backward of such an
   * input dropout: the masked product's output × its keep-bits × drop_scale. */
  const uint64_t* a_drop_seed;
  float a_drop_keep;
  float a_drop_scale;
} hgd_gemm_rows_desc;
hgd_status hgd_gemm_rows(const hgd_gemm_rows_desc* descs, int32_t count, void* stream);

typedef struct hgd_gemm_tn_desc {
  const float* A;
  int64_t lda;
  const float* relu_mask; /* [rows, M] or NULL */
  int64_t ldm;
  const float* B;
  int64_t ldb;
  int64_t rows;
  int32_t M;
  int32_t N;
  float* C;               /* [M, N] */
  float* colsum_A;        /* [M] or NULL */
  int32_t binarize_a;     /* A' = (A > 0 ? 1 : 0) instead of A (colsum_A then counts nonzeros) */
  const float* b_row_scale; /* [rows] or NULL: B's row r × b_row_scale[r] as it is loaded (the
                             * vertex means D_v^-1 of the mean two-hop's backward) */
  float c_scale;          /* 0 = off: C and colsum_A × c_scale as they are stored */
  /* b_drop_seed (NULL = off): nn.Dropout on B as it is loaded (element row·N + n kept as
   * hgd_dropout_apply keeps it, rows·N < 2^32, kept × b_drop_scale; before b_row_scale) — the
   * weight gradient of a Linear whose input dropout ran inside its forward */
  const uint64_t* b_drop_seed;
  float b_drop_keep;
  float b_drop_scale;
} hgd_gemm_tn_desc;
size_t hgd_gemm_tn_workspace_size(const hgd_gemm_tn_desc* descs, int32_t count);
hgd_status hgd_gemm_tn(const hgd_gemm_tn_desc* descs, int32_t count, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused InfoNCE, contrastLoss of util/loss_torch.py:103-110:
 *   p1 = normalize(E1[nodes] + 1e-8), p2 = normalize(E2[nodes] + 1e-8)   (eps 1e-12)
 *   loss = -(1/B) Σ_b log( exp(<p1_b,p2_b>/τ) / (Σ_j exp(<p1_b,p2_j>/τ) + 1e-8) )
 * Only the B batch rows are gathered and normalised; the [B, B] exp-sum is never materialised.
 * nodes follow torch indexing: negative ids count from the end of the table (HCCF.py:65-66 passes
 * torch.unique(emb.long())); ids outside [-n_rows, n_rows) are the caller's error (clamped here).
 * Forward writes P1, P2 [B, d] (contiguous), inv_norm1/2 [B], pos_logit [B], deno [2, B] and
 * the scalar loss (all device): deno[b] = Σ_j exp(<p1_b,p2_j>/τ) + 1e-8 and deno[B + b] = its
 * off-diagonal part (Σ_{j≠b} … + 1e-8), from which the loss term and the diagonal gradient
 * weight 1 − p_bb are formed without cancellation (p_bb rounds to 1 in fp32 for a one-node list;
 * the reference's fp32 autograd returns rounding noise there). B is the capacity for the _n
 * forms. Backward recomputes the logits and writes dX1, dX2 [B, d] =
 * dloss/d(E1[nodes]), dloss/d(E2[nodes]) scaled by the device scalar *grad_loss; scattering
 * them into the [N, d] table gradients (duplicate nodes add) is the caller's. d: multiple of 16
 * in [16, 256]. Deterministic (fixed-order reductions). Workspace: hgd_infonce_workspace_size.
 * ---------------------------------------------------------------------------------------- */
size_t hgd_infonce_workspace_size(int64_t batch, int32_t d);
hgd_status hgd_infonce_forward(const float* E1, int64_t ld1, const float* E2, int64_t ld2,
                               int64_t n_rows, const int64_t* nodes, int64_t batch, int32_t d,
                               float temp, float* P1, float* P2, float* inv_norm1,
                               float* inv_norm2, float* pos_logit, float* deno, float* loss,
                               void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_infonce_backward(const float* P1, const float* P2, const float* inv_norm1,
                                const float* inv_norm2, const float* deno, int64_t batch,
                                int32_t d, float temp, const float* grad_loss, float* dX1,
                                float* dX2, void* workspace, size_t workspace_bytes,
                                void* stream);
/* The same with the batch size held on the device (*batch_count <= capacity; the node list
 * is capacity-sized, e.g. a device-side unique whose count is never read back): grids and
 * strides use `capacity`, the kernels read the live count, rows past it come out as zeros
 * (P1/P2/dX1/dX2) and the mean divides by the live count. Nothing is read to the host, so a
 * training step using them can be captured in a HIP graph. Workspace:
 * hgd_infonce_workspace_size(capacity, d). */
hgd_status hgd_infonce_forward_n(const float* E1, int64_t ld1, const float* E2, int64_t ld2,
                                 int64_t n_rows, const int64_t* nodes, int64_t capacity,
                                 const int64_t* batch_count, int32_t d, float temp, float* P1,
                                 float* P2, float* inv_norm1, float* inv_norm2, float* pos_logit,
                                 float* deno, float* loss, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* Backward with the scatter fused: the gradient rows are added straight into the [n_rows, d]
 * table gradients dE1 / dE2 (zero-filled by the caller; either may be NULL: that side is not
 * computed) at
 * the batch rows' nodes (torch indexing, negative ids wrap), rows past *batch_count add nothing.
 * Atomic adds, but at most two batch rows meet on one table row, so the result is
 * deterministic. */
hgd_status hgd_infonce_backward_n(const float* P1, const float* P2, const float* inv_norm1,
                                  const float* inv_norm2, const float* deno, int64_t capacity,
                                  const int64_t* batch_count, int32_t d, float temp,
                                  const float* grad_loss, const int64_t* nodes, int64_t n_rows,
                                  float* dE1, int64_t ldE1, float* dE2, int64_t ldE2,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Several InfoNCE terms in ONE launch per kernel (HCCF's user and item terms of a layer,
 * HCCF.py:65-66): each term as hgd_infonce_forward_n / hgd_infonce_backward_n would take it
 * (batch_count NULL = all `capacity` rows live), with its own workspace
 * (hgd_infonce_workspace_size(capacity, d)). Backward outputs: dX1 / dX2 compact [capacity, d]
 * rows, or dE1 / dE2 scatter-adds into [n_rows, ld] tables (nodes required); a side without an
 * output is skipped. count is 1 to 8 (HCCF: the user and item terms of up to four layers, one
 * launch per kernel for the whole step's InfoNCE); all terms share d, temp and — backward —
 * grad_loss (the group's loss is the sum of its terms' losses). */
typedef struct hgd_infonce_term {
  const float* E1;
  int64_t ld1;
  const float* E2;
  int64_t ld2;
  int64_t n_rows;
  const int64_t* nodes;
  int64_t capacity;
  const int64_t* batch_count;
  float* P1;
  float* P2;
  float* inv_norm1;
  float* inv_norm2;
  float* pos_logit;
  float* deno;
  float* loss;
  float* dX1;
  float* dX2;
  float* dE1;
  int64_t ldE1;
  float* dE2;
  int64_t ldE2;
  void* workspace;
  size_t workspace_bytes;
} hgd_infonce_term;
hgd_status hgd_infonce_forward_group(const hgd_infonce_term* terms, int32_t count, int32_t d,
                                     float temp, void* stream);
hgd_status hgd_infonce_backward_group(const hgd_infonce_term* terms, int32_t count, int32_t d,
                                      float temp, const float* grad_loss, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ingest and graph build — the data path producing the hot path's
 * input matrices (data/loader.py:24-38, data/ui_graph.py:43-112, data/graph.py:11-25).
 *
 * Host (no GPU needed): hgd_ingest_read parses a "user<sep>item[<sep>…]" file exactly like
 * FileIO.load_data_set — first line skipped; a line with a tab splits on tabs, else on commas,
 * after stripping; fields 0/1 parsed like Python int(); other fields ignored; "\n", "\r\n" and
 * "\r" end lines — with n_threads parser threads (<= 0: all cores). Lines the reference would
 * reject fail the call (the message names the line). The handle owns the parsed arrays.
 * ---------------------------------------------------------------------------------------- */
typedef struct hgd_ingest hgd_ingest;
hgd_status hgd_ingest_read(const char* path, int32_t skip_header, int32_t n_threads,
                           hgd_ingest** out);
int64_t hgd_ingest_count(const hgd_ingest* h);  /* records, -1 for NULL */
/* Copies the raw user / item ids (host int64 arrays of hgd_ingest_count entries, file order). */
hgd_status hgd_ingest_copy(const hgd_ingest* h, int64_t* user_raw, int64_t* item_raw);
void hgd_ingest_free(hgd_ingest* h);

/* Device: ids[i] = rank of keys[i] among the distinct keys ordered by first appearance (the
 * `if user not in self.user: self.user[user] = len(self.user)` loop, data/ui_graph.py:43-56);
 * uniq[r] = the key with id r (first *n_unique entries); *n_unique on the device. */
size_t hgd_remap_workspace_size(int64_t n);
hgd_status hgd_remap_first_appearance(const int64_t* keys, int64_t n, int32_t* ids,
                                      int64_t* uniq, int64_t* n_unique, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* Device: canonical CSR (rows ascending, columns ascending, duplicates summed into float32
 * counts) of the COO (rows, cols) [n] — scipy csr_matrix((ones, (row, col))), ui_graph.py:70-84.
 * col_out / val_out need n entries; the nonzero count lands in device *nnz_out. */
size_t hgd_coo_coalesce_workspace_size(int64_t n);
hgd_status hgd_coo_coalesce(const int32_t* rows, const int32_t* cols, int64_t n, int64_t n_rows,
                            int64_t n_cols, int64_t* rowptr, int32_t* col_out, float* val_out,
                            int64_t* nnz_out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Device: out[e] = (row_scale[r]·val[e])·col_scale[col[e]] (col_scale NULL: no second factor) —
 * d_mat_inv.dot(adj).dot(d_mat_inv) of Graph.normalize_graph_mat with the scales of
 * hgd_degree_scale (power -0.5 square, -1 rectangular). */
hgd_status hgd_normalize_values(const int64_t* rowptr, const int32_t* col, const float* val,
                                int64_t n_rows, const float* row_scale, const float* col_scale,
                                float* out, void* stream);

/* Device: Knowledge.construct_data's triple table (data/knowledge.py:44-72) from the raw KG
 * (h, r, t) [n] and the CF pairs (cf_u, cf_i) [n_cf], int64. With n0 = max(r) + 1 (0 for an
 * empty KG) the 3n + 2·n_cf output rows are, in the reference's order:
 *   (h, r+2, t) | (t, r+n0+2, h) | (t, r+n0, h) | (cf_u, 0, cf_i) | (cf_i, 1, cf_u)
 * written as int64 (h_out, r_out, t_out) and as int32 copies for the sorts. stats (device
 * int64[4]) = { max(h,t)+1, max(h,t,cf_u,cf_i)+1, n0, #inputs that are negative or too large
 * for the int32 copies }: the copies are valid only when stats[3] == 0. */
hgd_status hgd_kg_expand(const int64_t* h, const int64_t* r, const int64_t* t, int64_t n,
                         const int64_t* cf_u, const int64_t* cf_i, int64_t n_cf, int64_t* h_out,
                         int64_t* r_out, int64_t* t_out, int32_t* h32_out, int32_t* r32_out,
                         int32_t* t32_out, int64_t* stats, void* stream);

/* ------------------------------------------------------------------------------------------
 * Structure primitives (all deterministic; indices bit-exact with the CPU restatement).
 * ---------------------------------------------------------------------------------------- */
/* int64 indices → int32, checking 0 <= v < upper; err_count (device int64) += #violations. */
hgd_status hgd_index_narrow(const int64_t* in, int64_t n, int64_t upper, int32_t* out,
                            int64_t* err_count, void* stream);
/* Stable sort of int32 keys in [0, n_keys): keys_out = sorted keys, perm_out[i] = source position. */
size_t hgd_sort_perm_workspace_size(int64_t n);
hgd_status hgd_sort_perm(const int32_t* keys, int64_t n, int64_t n_keys, int32_t* keys_out,
                         int32_t* perm_out, void* workspace, size_t workspace_bytes,
                         void* stream);
/* rowptr[r] = first position p with sorted_rows[p] >= r, r in [0, n_rows]. */
hgd_status hgd_rowptr_from_sorted(const int32_t* sorted_rows, int64_t nnz, int64_t n_rows,
                                  int64_t* rowptr, void* stream);
/* Counts positions where sorted_rows decreases or leaves [0,n_rows) into device int64 *bad. */
hgd_status hgd_check_sorted(const int32_t* rows, int64_t nnz, int64_t n_rows, int64_t* bad,
                            void* stream);
/* rows_out[e] = r for e in [rowptr[r], rowptr[r+1]), nnz = rowptr[n_rows]. */
hgd_status hgd_expand_rows(const int64_t* rowptr, int64_t n_rows, int64_t nnz, int32_t* rows_out,
                           void* stream);
/* out[i] = src[perm[i]] (4-byte elements: int32 or fp32 bit patterns). */
hgd_status hgd_gather32(const void* src, const int32_t* perm, int64_t n, void* out,
                        void* stream);
/* out[i] = src[perm[i]] for bytes: a CSR-order keep-mask into CSC order through perm_t
 * (hgd_spmm_masked's backward hop). perm 16-byte aligned, out 4-byte aligned. */
hgd_status hgd_gather_u8(const uint8_t* src, const int32_t* perm, int64_t n, uint8_t* out,
                         void* stream);
/* s[r] = deg(r)^power with deg = rowptr diff (val == NULL) or Σ val over the row; deg == 0 → 0.
 * power is -1.0 (D^-1) or -0.5 (D^-1/2) or any other exponent. */
hgd_status hgd_degree_scale(const int64_t* rowptr, const float* val, int64_t n_rows,
                            double power, float* scale_out, void* stream);
/* out[e] = (base ? base[perm ? perm[e] : e] : 1) * (src_scale ? src_scale[src_idx[e]] : 1). */
hgd_status hgd_edge_values(const float* base, const int32_t* perm, const float* src_scale,
                           const int32_t* src_idx, int64_t n, float* out, void* stream);

/* Drop-edge compaction (SpAdjDropEdge): keeps entries with mask[e] != 0 in order,
 * out_val = val[e] / keep. Writes the kept count to device int64 *out_count. */
size_t hgd_dropedge_workspace_size(int64_t nnz);
hgd_status hgd_dropedge_compact(const int64_t* rows, const int64_t* cols, const float* val,
                                const uint8_t* mask, int64_t nnz, float keep,
                                int64_t* out_rows, int64_t* out_cols, float* out_val,
                                int64_t* out_count, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Device keep-mask for drop-edge: mask[i] = floor(u_i + keep) != 0 with u_i a 24-bit uniform
 * from a counter-based hash of (seed, i) — the SpAdjDropEdge expression (HCCF.py:223) without
 * the host RNG round trip (statistically, not bitwise, equal to torch's CPU stream). */
hgd_status hgd_bernoulli_mask(uint64_t seed, int64_t n, float keep, uint8_t* mask, void* stream);
/* The same draw with the 64-bit seed read from device memory (seed[0]): a captured training step
 * advances the counter on the device, so every graph replay draws a fresh mask. */
hgd_status hgd_bernoulli_mask_dev(const uint64_t* seed, int64_t n, float keep, uint8_t* mask,
                                  void* stream);
/* The same draw for both orientations of a structure (hgd_spmm_masked's forward and backward
 * hops): mask[i] as hgd_bernoulli_mask_dev, mask_t[j] = mask[perm_t[j]] computed from the hash
 * of perm_t[j] (perm_t: CSC position → CSR position) instead of a byte gather. */
hgd_status hgd_bernoulli_mask_dev_pair(const uint64_t* seed, const int32_t* perm_t, int64_t n,
                                       float keep, uint8_t* mask, uint8_t* mask_t, void* stream);
/* Zeroes entries [*count, capacity) of the capacity-sized outputs of hgd_dropedge_structure
 * (count = rowptr_out + n_rows, on the device): a dropped structure whose kept count is never read
 * back keeps full-size arrays with a defined tail (index 0, weight 0). Null arrays are skipped. */
hgd_status hgd_dropedge_fill_tail(const int64_t* count, int64_t capacity, int32_t* col,
                                  float* val, int32_t* row_t, float* val_t, void* stream);

/* Sort-free rebuild of a drop-edge'd structure from its parent: compacts the parent CSR with the
 * mask (CSR order) and the parent CSC with mask[perm_t[e']] (perm_t: CSC position → CSR
 * position), dividing values by keep; row pointers are remapped through the prefix sums.
 * Outputs are sized for nnz (upper bound); the kept count is rowptr_out[n_rows]. No host sync. */
size_t hgd_dropedge_structure_workspace_size(int64_t nnz);
hgd_status hgd_dropedge_structure(const int64_t* rowptr, const int32_t* col, const float* val,
                                  const int64_t* colptr, const int32_t* row_t, const float* val_t,
                                  const int32_t* perm_t, int64_t n_rows, int64_t n_cols,
                                  int64_t nnz, const uint8_t* mask, float keep,
                                  int64_t* rowptr_out, int32_t* col_out, float* val_out,
                                  int64_t* colptr_out, int32_t* row_t_out, float* val_t_out,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* torch.nonzero(H > thresh) (mode HGD_DENSE_GREATER) or torch.nonzero(H) (HGD_DENSE_NONZERO)
 * of a dense row-major [n_rows, n_cols] fp32 matrix (leading dim ld), in two passes: rowptr
 * (n_rows+1, int64), then the column list (rowptr[n_rows] int32 entries) and, if vals != NULL,
 * the kept values in the same order. */
#define HGD_DENSE_GREATER 0
#define HGD_DENSE_NONZERO 1
size_t hgd_dense_threshold_workspace_size(int64_t n_rows);
hgd_status hgd_dense_threshold_rowptr(const float* H, int64_t n_rows, int64_t n_cols, int64_t ld,
                                      float thresh, int32_t mode, int64_t* rowptr,
                                      void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_dense_threshold_fill(const float* H, int64_t n_rows, int64_t n_cols, int64_t ld,
                                    float thresh, int32_t mode, const int64_t* rowptr,
                                    int32_t* cols, float* vals, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation (GraphRecommender.test, base/graph_recommender.py:61-92).
 *   hgd_mask_scores: scores[r, cols[rowptr[m]:rowptr[m+1]]] = value, m = row_map ? row_map[r] : r
 *                    (rated items → -10e8, :79-80).
 *   hgd_topk_rows:   per row, the K entries find_k_largest (util/algorithm.py:143-173) returns —
 *                    first K of {(c_j, j): j < K} ∪ {(c_i, i)} by score desc, seed first, index
 *                    asc (so top items among the first K appear twice, as in the reference).
 *                    1 <= k <= 256, n_cols >= k; out_ids int32 [n_rows, k], out_scores fp32.
 * ---------------------------------------------------------------------------------------- */
hgd_status hgd_mask_scores(float* scores, int64_t n_rows, int64_t ld, const int64_t* rowptr,
                           const int32_t* cols, const int32_t* row_map, float value,
                           void* stream);
hgd_status hgd_topk_rows(const float* scores, int64_t n_rows, int64_t n_cols, int64_t ld,
                         int32_t k, int32_t* out_ids, float* out_scores, void* stream);

/* Fused score, mask and top-K (GraphRecommender.test, base/graph_recommender.py:61-92, and
 * find_k_largest, util/algorithm.py:143-173): from the two fp32 embedding tables and the
 * rated-items CSR straight to the [n_rows, k] lists; no score is written to memory.
 *   Row r ranks user u = users ? users[r] : r (device int32, ids of user_emb rows).
 *   raw(u, i)  = the fp32 value the kernel's product gives for user_emb[u, :d]·item_emb[i, :d]
 *                (f32 MFMA: exact products, fp32 sums; within 1e-5·Σ_j|u_j·v_j| of the float64
 *                dot product).
 *   eff(u, i)  = mask_value if i is in rated_cols[rated_rowptr[u] : rated_rowptr[u+1]], else
 *                raw(u, i) (a rated item with a lower raw score is raised to mask_value, as
 *                hgd_mask_scores does); rated_rowptr == NULL masks nothing.
 *   Output: exactly what hgd_topk_rows returns for the row of effective scores — the first k of
 *   {(c_j, j): j < k} ∪ {(c_i, i)} by score descending, seed before stream, index ascending
 *   (seed duplicates listed; ±0.0 compare equal and the listed score keeps its sign).
 *   out_ids int32 / out_scores fp32, dense [n_rows, k].
 *   Position independence: a pair's raw score is one fixed instruction sequence over d (padded
 *   with zeros), so its bits do not depend on the row r, the tile, the segment, the launch or
 *   n_segments: a user listed twice gets identical rows, every n_segments gives identical output
 *   and every call repeats bitwise.
 *   rated_cols ascending within each row is a precondition (duplicates allowed); an unsorted row
 *   may give a wrong list but never an out-of-range access. users[r] and the rated rows must be
 *   valid indices of their tables.
 *   Any ldu, ldi >= d and any 4-byte-aligned base are accepted; item rows that are 16-byte
 *   aligned (base and ldi) take vector loads.
 *   n_segments splits the item range over that many workgroups per block of users (a handful of
 *   users still fills the chip); it is clamped to the tile count and to 256. 0 chooses from
 *   n_rows, n_items and a constant CU count of 256 — no device query, so the choice and the
 *   workspace size are pure functions of the arguments. The segments are merged by a second
 *   launch: no workgroup waits for another.
 *   No host synchronisation and no allocation: capturable.
 *   Before the first HIP call: null tables or outputs, d < 1, k < 1, k > n_items, ld < d,
 *   n_segments < 0, n_items >= 2^31 → HGD_ERR_INVALID_ARG; k > HGD_RANK_MAX_K, d > HGD_RANK_MAX_D
 *   or n_rows >= 2^31 → HGD_ERR_UNSUPPORTED; a workspace shorter than
 *   hgd_rank_topk_workspace_size (same arguments) → HGD_ERR_WORKSPACE; n_rows == 0 → HGD_OK with
 *   nothing launched.
 *   hgd_rank_topk_geometry (host only): the kernel's tiling, for tests and tools. */
#define HGD_RANK_MAX_K 64
#define HGD_RANK_MAX_D 256
void hgd_rank_topk_geometry(int32_t* users_per_block, int32_t* items_per_tile,
                            int32_t* candidate_slots);
size_t hgd_rank_topk_workspace_size(int64_t n_rows, int64_t n_items, int32_t k,
                                    int32_t n_segments);
hgd_status hgd_rank_topk(const float* user_emb, int64_t ldu, const float* item_emb, int64_t ldi,
                         int64_t n_items, int32_t d, const int32_t* users, int64_t n_rows,
                         const int64_t* rated_rowptr, const int32_t* rated_cols,
                         float mask_value, int32_t k, int32_t n_segments,
                         int32_t* out_ids, float* out_scores,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Per-user inputs of ranking_evaluation (util/evaluation.py:169-196) for the lists above:
 *   hits[r, c] = |set(test items of r) ∩ set(ids[r, :N_c])|        (Metric.hits, :8-15)
 *   dcg[r, c]  = Σ_{n < N_c, ids[r, n] in test} discount[n], in n order (Metric.NDCG, :84-97)
 * ids int32 [n_rows, ld] (device, k <= 256 used per row, negative = never a hit); the test items
 * of row r are test_cols[test_rowptr[r] : test_rowptr[r+1]] (device, ascending, distinct
 * internal item ids); discount float64 [k] (device) = 1.0/math.log(n+2, 2) computed by the host
 * so DCG is bit-identical to the reference; cutoffs = the N values (HOST array, ascending, in
 * [1, k], at most 16). Outputs hits int32 / dcg float64 [n_rows, n_cutoffs].
 * All three entries: n_rows = 0 launches nothing; n_rows > 2^31 - 1 is HGD_ERR_UNSUPPORTED. */
hgd_status hgd_rank_metrics(const int32_t* ids, int64_t n_rows, int64_t ld, int32_t k,
                            const int64_t* test_rowptr, const int32_t* test_cols,
                            const int32_t* cutoffs, int32_t n_cutoffs, const double* discount,
                            int32_t* hits, double* dcg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pairwise training sampler (HOST functions, host pointers): next_batch_pairwise
 * (util/sampler.py:237-264) with CPython's random module bit for bit. mt_state = the 625 words
 * of random.getstate()[1] (624 MT19937 words + position), read and advanced in place — the
 * caller hands it back with random.setstate, so the Python stream continues exactly as if the
 * reference loop had run.
 *   hgd_py_shuffle:      random.shuffle(x) applied to order[0..n) (x[k] = record order[k]).
 *   hgd_sample_pairwise: records order[begin..end): out_u / out_i = rec_user / rec_item of the
 *                        record, then n_negs draws choice(item_list) per record (dense id =
 *                        _randbelow(n_items)), redrawn while in the user's training items
 *                        user_items[user_rowptr[u] : user_rowptr[u+1]] (ascending);
 *                        out_j [(end-begin) * n_negs]. Fails (instead of looping forever like the
 *                        reference) for a user who has every item.
 * ---------------------------------------------------------------------------------------- */
hgd_status hgd_py_shuffle(uint32_t* mt_state, int64_t* order, int64_t n);
hgd_status hgd_sample_pairwise(uint32_t* mt_state, const int64_t* order, int64_t begin,
                               int64_t end, const int32_t* rec_user, const int32_t* rec_item,
                               const int64_t* user_rowptr, const int32_t* user_items,
                               int64_t n_users, int64_t n_items, int32_t n_negs, int32_t* out_u,
                               int32_t* out_i, int32_t* out_j);

/* ------------------------------------------------------------------------------------------
 * Unified CF + KG training sampler (HOST functions, host pointers): next_batch_unified
 * (util/sampler.py:7-90), consuming Python's random stream and NumPy's legacy global
 * RandomState bit for bit. Both states are the 625 words (624 MT19937 words + position) that
 * random.getstate()[1] and np.random.get_state()[1:3] expose, advanced in place.
 *   hgd_py_shuffle_rows: random.shuffle(x) on a 2-D NumPy array. Its rows are views, so the swap
 *                        `x[i], x[j] = x[j], x[i]` degenerates to x[i] = x[j]: order[i] =
 *                        order[j], a resample with repeated rows. order NULL: only the n - 1
 *                        draws are consumed (the reference's shuffle(kg_data)).
 *   hgd_sample_unified:  one batch. (1) The CF part exactly as hgd_sample_pairwise over records
 *                        order[begin..end), int64 outputs. (2) batch_kg positions
 *                        np.random.randint(n_sel): masked rejection on 32-bit outputs of np_state
 *                        (none when n_sel == 1); position v yields head sel_head[v] (the head's
 *                        position in the epoch's head order, or head_ids[that] when head_ids is
 *                        given), sel_rel[v], sel_tail[v]. (3) per drawn triple, in order,
 *                        all_tails[_randbelow(n_tails)] from py_state, redrawn while in the
 *                        head's tails tail_sorted[tail_rowptr[p] : tail_rowptr[p+1]] (ascending,
 *                        distinct). n_sel == 0 is an error (NumPy raises); a head holding every
 *                        tail fails instead of looping forever like the reference.
 * ---------------------------------------------------------------------------------------- */
typedef struct hgd_unified_batch {
  uint32_t* py_state;
  uint32_t* np_state;
  /* CF part: as hgd_sample_pairwise */
  const int64_t* order;
  int64_t begin, end;
  const int32_t* rec_user;
  const int32_t* rec_item;
  const int64_t* user_rowptr;
  const int32_t* user_items;
  int64_t n_users, n_items;
  int32_t n_negs;
  int32_t reserved;
  /* KG part: the epoch's tables */
  const int64_t* sel_head; /* [n_sel] head position in [0, n_heads) */
  const int64_t* sel_rel;  /* [n_sel] */
  const int64_t* sel_tail; /* [n_sel] */
  int64_t n_sel;
  const int64_t* head_ids; /* [n_heads] entity id of a position, or NULL */
  const int64_t* all_tails; /* [n_tails] */
  int64_t n_tails;
  const int64_t* tail_rowptr; /* [n_heads + 1] */
  const int64_t* tail_sorted;
  int64_t n_heads;
  int64_t batch_kg;
  /* outputs: [end - begin], [end - begin], [(end - begin) * n_negs], then 4 × [batch_kg] */
  int64_t* out_u;
  int64_t* out_i;
  int64_t* out_j;
  int64_t* out_h;
  int64_t* out_r;
  int64_t* out_t;
  int64_t* out_n;
} hgd_unified_batch;
hgd_status hgd_py_shuffle_rows(uint32_t* mt_state, int64_t* order, int64_t n);
hgd_status hgd_sample_unified(const hgd_unified_batch* batch);

/* SpAdjDropEdge's CPU keep-mask (HCCF.py:223: floor(torch.rand(nnz) + keepRate).bool()) from
 * torch's default CPU generator, bit for bit, in one host pass (HOST function). torch_state =
 * the bytes of torch.get_rng_state() (hgd_torch_cpu_state_bytes(), 5056 on x86-64), advanced in
 * place by n draws for torch.set_rng_state; mask uint8 [n] (host); *kept = number of ones.
 * Long draws are split over host threads (HGD_TUNE_CPU_RNG_THREADS), each starting from the
 * MT19937 state its first draw sees, computed by a GF(2) jump-ahead: the same bits as one thread. */
size_t hgd_torch_cpu_state_bytes(void);
hgd_status hgd_torch_cpu_keep_mask(uint8_t* torch_state, int64_t state_bytes, int64_t n,
                                   float keep, uint8_t* mask, int64_t* kept);
/* The same with an explicit host thread count (0 = HGD_TUNE_CPU_RNG_THREADS' default): a draw
 * that runs beside a host-bound eager step should leave cores to it. */
hgd_status hgd_torch_cpu_keep_mask_threads(uint8_t* torch_state, int64_t state_bytes, int64_t n,
                                           float keep, uint8_t* mask, int64_t* kept,
                                           int32_t threads);
/* Test hook: 1 if the jump-ahead reproduces `refills` MT19937 refills of a seeded state. */
int32_t hgd_torch_cpu_jump_selfcheck(int64_t refills);

/* ------------------------------------------------------------------------------------------
 * Sorted unique of integer keys — torch.unique(t.long()) as HCCF's loss calls it every step on
 * [batch, d] embedding blocks: contrastLoss(..., torch.unique(ancs.long()), ...),
 * model/graph/HCCF.py:65-66 (the truncated embedding values become the node list).
 *   hgd_unique_i64 / hgd_unique_trunc_f32: range-bitmap path, no host sync. out [n] receives the
 *     distinct keys ascending (the trunc variant truncates floats toward zero like Tensor.long();
 *     NaN / ±inf / |x| >= 2^63 become INT64_MIN), device *n_out their count — or -1 when the
 *     key range exceeds 2^24, in which case the caller runs the matching hgd_unique_sort_* (device
 *     radix sort + unique, same output). n < 2^31. Workspace: hgd_unique_workspace_size(n).
 * ---------------------------------------------------------------------------------------- */
size_t hgd_unique_workspace_size(int64_t n);
hgd_status hgd_unique_i64(const int64_t* keys, int64_t n, int64_t* out, int64_t* n_out,
                          void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_unique_trunc_f32(const float* x, int64_t n, int64_t* out, int64_t* n_out,
                                void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_unique_sort_i64(const int64_t* keys, int64_t n, int64_t* out, int64_t* n_out,
                               void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_unique_sort_trunc_f32(const float* x, int64_t n, int64_t* out, int64_t* n_out,
                                     void* workspace, size_t workspace_bytes, void* stream);
/* Device-complete form (a captured training step cannot take the host-side fallback): the
 * bitmap window is [min, min + 2^24); keys beyond it are collected and sorted by one workgroup
 * (in LDS up to 4,096 of them, else a bitonic network over the workspace) and appended — they
 * are all larger. *n_out is always the unique count. Same output as the forms above.
 * n in [0, 2^29] (HGD_ERR_INVALID_ARG beyond): every key but the smallest may be a far key, and
 * the far sort counts them, their padded power of two P and the bitonic pass size, which
 * reaches 2·P, in 32-bit ints. */
hgd_status hgd_unique_dev_i64(const int64_t* keys, int64_t n, int64_t* out, int64_t* n_out,
                              void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_unique_dev_trunc_f32(const float* x, int64_t n, int64_t* out, int64_t* n_out,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Several lists through the device-complete path at once (HCCF's anchor and positive node
 * lists, HCCF.py:65-66): one launch per kernel for all of them, each list's out / n_out exactly
 * as hgd_unique_dev_i64 / hgd_unique_dev_trunc_f32 give it. Per list: exactly one of x_f32
 * (truncated like Tensor.long()) and x_i64, and its own workspace of
 * hgd_unique_workspace_size(n) bytes. `capacity` (0 = n): *n_out is clamped to it and
 * out[*n_out, capacity) zeroed — a fixed-size list whose live count stays on the device (the
 * capacity-sized node lists HCCF's InfoNCE reads). count is 1 to 4; per list n in [0, 2^29] and
 * capacity in [0, n] (HGD_ERR_INVALID_ARG otherwise). */
typedef struct hgd_unique_job {
  const float* x_f32;
  const int64_t* x_i64;
  int64_t n;
  int64_t capacity;
  int64_t* out;
  int64_t* n_out;
  void* workspace;
  size_t workspace_bytes;
} hgd_unique_job;
hgd_status hgd_unique_dev_group(const hgd_unique_job* jobs, int32_t count, void* stream);

/* ------------------------------------------------------------------------------------------
 * BPR loss from the embedding table (util/loss_torch.py:5-9 over the rows HCCF.py:84-86
 * gathers): E [n_users + n_items, lde] (users first, 16-byte aligned rows, d % 4 == 0,
 * d <= 256); anc = E[uid], pos = E[n_users + pid], neg = E[n_users + nid] (int64 ids, torch
 * indexing semantics; out-of-range ids are clamped, never dereferenced, and the forward adds
 * the number of batch rows holding one to *bad_index when it is non-NULL — a device word the
 * caller zeroes and reads when it chooses: the reference's gather raises on such an id);
 *   loss = mean_k −log(1e-5 + σ(⟨anc_k,pos_k⟩ − ⟨anc_k,neg_k⟩)), coef_k = σ(1−σ)/(1e-5+σ).
 * anc_out / pos_out ([batch, d], optional) receive the gathered rows (HCCF's InfoNCE node lists
 * are taken from them). Backward: dE = ∂(grad·loss)/∂E written in full (zero rows included;
 * `grad` a device scalar), every touched row summed over its positions in a fixed order
 * (position order for rows with at most 8 positions; rows with more — a skewed catalogue's
 * popular items — by one workgroup in fixed contiguous ranges of their ascending positions,
 * combined in range order): deterministic, integer atomics only.
 * Workspace: hgd_bpr_workspace_size(batch, n_rows). */
size_t hgd_bpr_workspace_size(int64_t batch, int64_t n_rows);
hgd_status hgd_bpr_forward(const float* E, int64_t lde, int64_t n_users, int64_t n_items,
                           int32_t d, const int64_t* uid, const int64_t* pid, const int64_t* nid,
                           int64_t batch, float* anc_out, float* pos_out, float* coef,
                           float* loss, int32_t* bad_index, void* workspace,
                           size_t workspace_bytes, void* stream);
hgd_status hgd_bpr_backward(const float* E, int64_t lde, int64_t n_users, int64_t n_items,
                            int32_t d, const int64_t* uid, const int64_t* pid,
                            const int64_t* nid, int64_t batch, const float* coef,
                            const float* grad, float* dE, int64_t ldd, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise epilogues around the hops (contiguous fp32, 16-byte aligned).
 *   apply:    y = epi(z)                                   (nn.LeakyReLU / nn.ReLU forward)
 *   backward: dz = dy * (ref > 0 ? 1 : slope) for LEAKY, dy * (ref > 0) for RELU, where ref is
 *             the pre-activation (or the output when slope >= 0, which has the same sign).
 * ---------------------------------------------------------------------------------------- */
hgd_status hgd_epilogue_apply(const float* z, int64_t n, int32_t epilogue, float slope, float* y,
                              void* stream);
hgd_status hgd_epilogue_backward(const float* ref, const float* dy, int64_t n, int32_t epilogue,
                                 float slope, float* dz, void* stream);
/* nn.Dropout(p) on the library's counter-based RNG (the ED-HNN block's dropouts,
 * layers2/EquivSetGNN2.py:91-101, when they run in its Linear stores or alone): y[i] = x[i]·scale
 * if element i (< 2^32) is kept, else 0. Elements 4c .. 4c + 3 share one draw:
 * h1 = lowbias32(lowbias32(c + lo32(s)) ^ hi32(s)), h2 = lowbias32(h1 ^ 0x9E3779B9), s = *seed
 * (a device value); element 4c + j is kept iff the j-th 16-bit half of (h1, h2), low half
 * first, is below floor(keep·65536 + 0.5) (f32). keep = 1 - p, scale = 1 / (1 - p). The
 * backward is the same call on the gradient with the same seed (no mask is stored). x, y
 * 16-byte aligned; y may alias x. */
/* The backward of `count` nn.Dropout calls on one tensor (torch's native_dropout_backward per
 * call, g_k = ((float)mask_k · dy_k) · scale, then autograd's accumulation of the calls'
 * gradients as they arrive, the last call's first): out = ((g_{count-1} + g_{count-2}) + …) + g_0
 * in one pass, products and sums rounded separately (bitwise torch's kernels). Up to 8 calls per
 * job, up to 4 jobs (tensors) per launch; dy / out 16-byte aligned, masks (bool bytes) 4-byte
 * aligned. HCCF's hypergraph dropouts (HCCF.py:182-186, one per layer on each of E_u·W_u and
 * E_i·W_i) are two such jobs. */
typedef struct hgd_masked_sum {
  const float* dy[8];
  const uint8_t* mask[8];
  float* out;
  int64_t n;
  int32_t count;
  float scale;
} hgd_masked_sum;
hgd_status hgd_masked_scale_sum(const hgd_masked_sum* jobs, int32_t n_jobs, void* stream);
hgd_status hgd_dropout_apply(const float* x, int64_t n, const uint64_t* seed, float keep,
                             float scale, float* y, void* stream);
/* out[i] = Σ_s P[s·slice_stride + i] over s = 0..n_slices-1, summed in slice order (bitwise the
 * chain ((P_0 + P_1) + P_2) + …): HCCF's `sum(hidden)` (model/graph/HCCF.py:188) over the layer
 * tables kept as slices of one buffer. P, out 16-byte aligned, slice_stride % 4 == 0. */
hgd_status hgd_sum_slices(const float* P, int64_t n_slices, int64_t slice_stride, int64_t n,
                          float* out, void* stream);
/* out[i] = ((a_0[i] + a_1[i]) + a_2[i]) + … over n_arrays (1..8) separate device arrays of
 * `count` floats, in array order, one pass: the gradient of a table used by several layers
 * (HGNN_HD4.py:390-405's residual `res`, read by every layer) as one sum instead of a chain of
 * binary accumulations. `arrays` is a HOST array of device pointers; all 16-byte aligned; out
 * may alias a_0. */
hgd_status hgd_sum_arrays(const float* const* arrays, int32_t n_arrays, int64_t count,
                          float* out, void* stream);

/* The reference's optimizer step, torch.optim.Adam(params, lr=…) (model/graph/HCCF.py:33; the
 * multi-tensor non-capturable form torch runs on the device, no weight decay / amsgrad), as ONE
 * kernel over up to 16 tensors — capturable, since its per-step scalars are read from the device
 * table `scalars` ([rows, count, 6] floats: 1 − β1, β2, 1 − β2, sqrt(1 − β2^t), eps,
 * −lr / (1 − β1^t), each the float of the double torch computes on the host, one row per step):
 * row *step_row is used and then step_row is advanced on the device (a second, one-thread
 * launch on the same stream), so a graph holding the call steps through the table by itself;
 * step_row NULL reads row 0 and advances nothing. Per element, in torch's op order and rounding:
 * m ← m + w·(g − m); v ← v·β2; v ← v + value·(g·g); d ← sqrt(v)/c2 + eps; p ← p + s·(m/d).
 * `variant` (0..31) selects the fused multiply-adds (bits 0–2: lerp, addcmul, addcdiv) and the
 * approximate sqrt / division (bits 3, 4) the torch build on the image matches bit for bit
 * (tests/test_gpu_adam.py). `tensors` is a HOST array. */
typedef struct hgd_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
} hgd_adam_tensor;
hgd_status hgd_adam_step(const hgd_adam_tensor* tensors, int32_t count, const float* scalars,
                         int32_t* step_row, int32_t variant, void* stream);

/* ------------------------------------------------------------------------------------------
 * Incidence objects (SURVEY.md §8b "C ABI libhgd"): the library-owned form of the structure the
 * flat calls above take as loose arrays. One object holds H's CSR (rows = vertices / users,
 * columns = hyperedges / items), its CSC, the CSC→CSR permutation, the degree scales of both
 * sides and the split plans — what the reference's torch.sparse COO `adj` plus cuSPARSE's
 * per-call coalesce/transpose stand for (base/torch_interface.py:8-12, HGNN_HD4.py:455-462).
 *
 *   hgd_incidence_create      convert_sparse_mat_to_tensor + the per-call adj.t() / coalesce
 *   hgd_incidence_from_dense  torch.nonzero(H > 0) of EquivSetGNN2.generate_V_E
 *                             (layers2/EquivSetGNN2.py:105-133) and DHCF's dense adjacency
 *   hgd_incidence_dropedge    SpAdjDropEdge.forward (HCCF.py:213-226) without a sort
 *   hgd_incidence_spmm        torch.sparse.mm(adj, X) / torch.sparse.mm(adj.t(), X)
 *   hgd_conv2hop_forward/     HGCNConv.forward (HGNN_HD4.py:455-462), the ED-HNN scatter-mean
 *   hgd_conv2hop_backward     pair (layers2/EquivSetConv2.py:88-93), HGNN normalisation
 *                             (data/graph.py:28-42) and their autograd backward
 *
 * Creation and drop-edge are setup calls: they allocate device memory (hipMalloc) and
 * synchronise `stream` once (split-plan and kept counts). The object is then immutable apart
 * from lazily built per-nonzero weights (guarded by an internal mutex; hgd_incidence_prepare
 * builds them ahead of graph capture), so it may be used from several threads and streams
 * at once. The object owns its arrays; callers' buffers are only read.
 * ---------------------------------------------------------------------------------------- */
typedef struct hgd_incidence hgd_incidence;

/* Degree scales of one side of H (torch_scatter 'mean' = 1/deg, data/graph.py:11-25 and :28-42
 * D^-1/2 / D^-1 with inf→0; the W-variants use the weighted degree Σ val). */
typedef enum hgd_scale {
  HGD_SCALE_NONE = 0,
  HGD_SCALE_MEAN = 1,  /* deg^-1   */
  HGD_SCALE_SYM = 2,   /* deg^-1/2 */
  HGD_SCALE_WMEAN = 3, /* (Σ val)^-1   */
  HGD_SCALE_WSYM = 4   /* (Σ val)^-1/2 */
} hgd_scale;
#define HGD_SIDE_ROWS 0
#define HGD_SIDE_COLS 1

/* Copies the CSR (rowptr [n_rows+1] int64, col [nnz] int32, val [nnz] or NULL = binary; device
 * pointers) into a new object, validates it (rowptr monotone from 0 to nnz, 0 <= col < n_cols;
 * columns need not be sorted within a row) and derives the CSC (stable: rows ascending within a
 * column), scales and split plans. */
hgd_status hgd_incidence_create(const int64_t* rowptr, const int32_t* col, const float* val,
                                int64_t n_rows, int64_t n_cols, int64_t nnz,
                                hgd_incidence** out, void* stream);
/* The object of torch.nonzero(H > thresh) (HGD_DENSE_GREATER) or torch.nonzero(H)
 * (HGD_DENSE_NONZERO) of a dense [n_rows, n_cols] matrix (leading dim ld); keep_values != 0
 * keeps H's entries as values, otherwise the incidence is binary. */
hgd_status hgd_incidence_from_dense(const float* H, int64_t n_rows, int64_t n_cols, int64_t ld,
                                    float thresh, int32_t mode, int32_t keep_values,
                                    hgd_incidence** out, void* stream);
/* SpAdjDropEdge: the child keeps the nonzeros with keep_mask[e] != 0 (CSR order, nnz bytes) and
 * carries values val[e]/keep (a binary parent's values are 1, so the child's are 1/keep).
 * Built by compaction of the parent's CSR and CSC (no sort). A child cannot be dropped again
 * (the reference always drops the base adjacency). */
hgd_status hgd_incidence_dropedge(const hgd_incidence* parent, const uint8_t* keep_mask,
                                  float keep, hgd_incidence** out, void* stream);
void hgd_incidence_destroy(hgd_incidence* inc);

/* Read-only view of the object's device arrays (valid until destroy). */
typedef struct hgd_incidence_view {
  int64_t n_rows, n_cols, nnz;
  const int64_t* rowptr;  /* CSR */
  const int32_t* col;
  const float* val;       /* NULL: binary */
  const int64_t* colptr;  /* CSC */
  const int32_t* row_t;
  const float* val_t;
  const int32_t* perm_t;  /* CSC position → CSR position (NULL for a drop-edge child) */
} hgd_incidence_view;
hgd_status hgd_incidence_get_view(const hgd_incidence* inc, hgd_incidence_view* out);
/* Device pointer to the object's degree scale of one side (HGD_SIDE_ROWS / HGD_SIDE_COLS);
 * NULL for HGD_SCALE_NONE. The column scales are the global ones after
 * hgd_incidence_globalize_columns. */
hgd_status hgd_incidence_scale(const hgd_incidence* inc, int32_t side, int32_t kind,
                               const float** out);
/* Builds the per-nonzero weights conv2hop needs for source-side scales `kinds_mask`
 * (bit k = hgd_scale k) now, so that later calls allocate nothing (graph capture). */
hgd_status hgd_incidence_prepare(const hgd_incidence* inc, uint32_t kinds_mask, void* stream);

/* Workspace of hgd_incidence_spmm for width d (the split-plan partials). */
size_t hgd_incidence_workspace_size(const hgd_incidence* inc, int32_t d);
/* Y = epi(row_scale ⊙ (A·X)) (transpose = 0, Y has n_rows rows) or epi(row_scale ⊙ (Aᵀ·X))
 * (transpose = 1, served by the CSC, Y has n_cols rows); values are A's. row_scale: NULL or a
 * device array over Y's rows (e.g. from hgd_incidence_scale). */
hgd_status hgd_incidence_spmm(const hgd_incidence* inc, int32_t transpose, const float* X,
                              int64_t ldx, float* Y, int64_t ldy, int32_t d,
                              const float* row_scale, int32_t epilogue, float slope,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Multi-GPU exchange: one process per GPU, users (rows of H) sharded in
 * contiguous ranges, items (columns) replicated; RCCL over xGMI. The communicator owns a side
 * stream for the chunked, overlapped all-reduce of the item sums. */
typedef struct hgd_comm hgd_comm;
#define HGD_COMM_ID_BYTES 128
/* Rank 0 creates the id (host buffer of HGD_COMM_ID_BYTES) and distributes it out of band. */
hgd_status hgd_comm_get_unique_id(void* id_out);
/* Collective over the nranks processes; binds the communicator to the current HIP device. */
hgd_status hgd_comm_create(const void* id, int32_t nranks, int32_t rank, hgd_comm** out);
void hgd_comm_destroy(hgd_comm* comm);
/* Item chunks per exchange for the overlapped hop (default 4, 1..64; RCCL transport). */
hgd_status hgd_comm_set_chunks(hgd_comm* comm, int32_t n_chunks);
/* In-place sum of a device fp32 buffer over the ranks, ordered on `stream` (over the peer
 * exchange: count a multiple of 4 <= its max_count, buf 16-byte aligned; uses send slot 0). */
hgd_status hgd_exchange_allreduce(hgd_comm* comm, float* buf, int64_t count, void* stream);
/* Replaces the object's column degrees by their sum over the ranks (each rank holds a user
 * shard of the same item set), so column scales — the Q of conv2hop — are global. Collective;
 * synchronises `stream`. */
hgd_status hgd_incidence_globalize_columns(hgd_incidence* inc, hgd_comm* comm, void* stream);

/* Direct xGMI peer exchange (SURVEY.md §8e "mesh … direct hipIpc peer kernel"), an alternative
 * transport to RCCL for the same all-reduce of the item messages: a two-shot reduce over the
 * mesh — rank r sums block r of every rank's send slot (reading the N-1 peers over their own
 * xGMI links at once, ranks summed in ascending order), then gathers the other blocks from the
 * peers' reduced slots. Every rank exposes a flag page and 2·n_slots slots of max_count floats
 * (send, then reduced) in uncached segments of at most 1 GiB (HGD_TUNE_P2P_SEGMENT_MB), each
 * through hipIpcGetMemHandle. Setup is collective out of band: create, export, exchange the
 * handles (e.g. all_gather), open. Peer reads follow a system-scope acquire and announced
 * stores a system-scope release, so correctness does not depend on how the importing device
 * caches peer memory (csrc/p2p.hip, "Memory ordering").
 * Waits are bounded (hgd_p2p_set_timeout, default 30 s): a timeout sets a device error flag
 * and a host-visible copy; hgd_p2p_poll reports it without synchronising, hgd_p2p_check after
 * a sync, and every later exchange writes NaN into its output instead of summing.
 * A slot used by exchange i may be rewritten once any later exchange j > i has completed on
 * this rank's stream; every rank must issue the same exchanges in the same order.
 * Replaces: nothing in the reference (no distributed code, HCCF.py:24); the design's own. */
typedef struct hgd_p2p hgd_p2p;
#define HGD_P2P_HANDLE_BYTES 4096
/* A communicator whose exchanges run over an OPENED peer exchange instead of RCCL (no RCCL
 * communicator; `p2p` must outlive it and is not destroyed with it). conv2hop over it pipelines
 * column slices: hop 1 of a slice writes straight into a send slot, the slot's mesh reduce runs
 * on the communicator's high-priority side stream, hop 2 of the slice waits only for it (the
 * same slices, slots and kernels as sharded.ShardedIncidence with transport 'p2p'). Needs
 * d % 4 == 0 and 2·ceil(d / width) slots of n_cols·width floats. hgd_incidence_globalize_columns
 * over it sums the degrees exactly (16-bit limbs). */
hgd_status hgd_comm_create_p2p(hgd_p2p* p2p, int32_t nranks, int32_t rank, hgd_comm** out);
/* Column-slice width of the peer-exchange pipeline: 0 = default (32 for d <= 128, else 64),
 * else a multiple of 4. */
hgd_status hgd_comm_set_slice_width(hgd_comm* comm, int32_t width);
/* nranks 1..8; max_count a positive multiple of 4 (floats per slot, at most one segment);
 * n_slots 1..1024 (at most 62 segments in all). */
hgd_status hgd_p2p_create(int32_t nranks, int32_t rank, int64_t max_count, int32_t n_slots,
                          hgd_p2p** out);
void hgd_p2p_destroy(hgd_p2p* p2p);
/* This rank's handle (HGD_P2P_HANDLE_BYTES host bytes) for its peers. */
hgd_status hgd_p2p_export(const hgd_p2p* p2p, void* handle_out);
/* `handles`: nranks × HGD_P2P_HANDLE_BYTES in rank order (this rank's own entry included).
 * Checks that every imported mapping spans the peer's whole allocation. */
hgd_status hgd_p2p_open(hgd_p2p* p2p, const void* handles);
/* Device pointer of this rank's send slot (max_count floats; write the partial sums here). */
float* hgd_p2p_slot(hgd_p2p* p2p, int32_t slot);
int32_t hgd_p2p_n_slots(const hgd_p2p* p2p);
int64_t hgd_p2p_max_count(const hgd_p2p* p2p);
hgd_status hgd_p2p_set_timeout(hgd_p2p* p2p, double seconds);
/* out[0:count) = Σ_ranks send_slot[0:count), ordered on `stream`; count a multiple of 4 and
 * out 16-byte aligned. */
hgd_status hgd_p2p_allreduce(hgd_p2p* p2p, int32_t slot, int64_t count, float* out,
                             void* stream);
/* Synchronous: HGD_OK, or HGD_ERR_HIP if any exchange timed out. */
hgd_status hgd_p2p_check(hgd_p2p* p2p);
/* Non-blocking: HGD_ERR_HIP if a wait that has already run timed out (host-visible flag). */
hgd_status hgd_p2p_poll(const hgd_p2p* p2p);
/* Pricing hook: k_reduce (rank 0's block over nranks sources) and k_gather (the other blocks) of
 * a `count`-float exchange with every peer slot a separate LOCAL allocation (uncached unless
 * `cached`), mean ms per launch over `iters` launches; synchronises `stream`. Prices the
 * kernels, not xGMI (profiles/r04_scale). */
hgd_status hgd_p2p_price_local(int32_t nranks, int64_t count, int32_t cached, int32_t iters,
                               float* ms_reduce, float* ms_gather, void* stream);
/* The block arithmetic of hgd_p2p_allreduce (host only, no device calls): rank q reduces floats
 * [*lo, *hi) of a `count`-float exchange over `nranks` ranks; gather step i of `rank` copies
 * float4 *j from rank *owner's reduced block (its own block is skipped). */
hgd_status hgd_p2p_block_range(int64_t count, int32_t nranks, int32_t q, int64_t* lo,
                               int64_t* hi);
hgd_status hgd_p2p_gather_index(int64_t count, int32_t nranks, int32_t rank, int64_t i,
                                int64_t* j, int32_t* owner);

/* The two-hop conv over the object, Y = epi(P·A·Q·Aᵀ·R·X) with P, R row scales and Q a column
 * scale (hgd_scale each):
 *   HGCNConv (HGNN_HD4.py:455-462)        P = Q = R = NONE on the weighted norm_adj
 *   ED-HNN mean pair (EquivSetConv2:88-93) P = MEAN, Q = MEAN, R = NONE on the binary V/E incidence
 *   HGNN normalisation (graph.py:28-42)    P = SYM, Q = MEAN, R = SYM (the benchmarked op)
 * Forward: hop 1 M = Q·Aᵀ·(R·X) over the CSC into the workspace (copied to saved_M when not
 * NULL), hop 2 Y = epi(P·A·M) over the CSR. An activation with slope >= 0 is fused into hop 2;
 * with slope < 0, pre_act [n_rows, d] (contiguous) receives P·A·M and Y = epi(pre_act).
 * Backward: dZ = epi'(dY) (act_ref = the forward Y when slope >= 0, else pre_act; NULL without
 * an epilogue), dM = Q·Aᵀ·(P·dZ), dX = R·A·dM — the same hops with P and R swapped.
 * comm != NULL: this rank's A is a user shard; hop 1's item sums are all-reduced (chunked and
 * overlapped on the communicator's stream over RCCL, or column-sliced over the peer exchange of
 * hgd_comm_create_p2p) before hop 2; Q must be NONE or the global
 * MEAN / SYM of hgd_incidence_globalize_columns. Epilogues with slope < 0 or dY with ldy != d
 * need contiguous rows. Workspace: hgd_conv2hop_workspace_size. */
size_t hgd_conv2hop_workspace_size(const hgd_incidence* inc, int32_t d, int32_t epilogue);
hgd_status hgd_conv2hop_forward(const hgd_incidence* inc, int32_t P, int32_t Q, int32_t R,
                                const float* X, int64_t ldx, int32_t d, float* Y, int64_t ldy,
                                int32_t epilogue, float slope, float* saved_M, float* pre_act,
                                hgd_comm* comm, void* workspace, size_t workspace_bytes,
                                void* stream);
hgd_status hgd_conv2hop_backward(const hgd_incidence* inc, int32_t P, int32_t Q, int32_t R,
                                 const float* dY, int64_t ldy, int32_t d, const float* act_ref,
                                 int32_t epilogue, float slope, float* dX, int64_t ldx,
                                 hgd_comm* comm, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * KG attention: KHGRec's update_attention (model/graph/KHGRec.py:298-331, called on every
 * minibatch, :122) for a batch of B triples (h, t, r) without leaving the device. fp32, every
 * sum in a fixed order, no atomics: two runs are bitwise equal, and a triple's score does not
 * depend on its position in the batch.
 *
 * hgd_kg_attention_scores — Equation 4, update_attention_batch (KHGRec.py:298-307) and the
 * per-relation loop around it (:312-320: one torch.where, two gathers and two matmuls per
 * relation) as ONE launch:
 *   v[i] = Σ_k (E[t_i]·W_r)_k · tanh((E[h_i]·W_r)_k + R[r]_k),  r = r_i
 *   E: [n_ent, d] rows ldE apart; W: [n_rel, d, dr] contiguous (trans_M); R: [n_rel, dr] rows ldR
 *   apart (relation_emb); h, t: int32 [B] in the batch's order.
 *   grp_perm: int32 [B], the triples grouped by relation (hgd_sort_perm of r: position p of the
 *   grouped order is triple grp_perm[p]); rel_off: int64 [n_rel+1], relation r owns positions
 *   [rel_off[r], rel_off[r+1]) (hgd_rowptr_from_sorted). A workgroup takes 32 triples of one
 *   relation and reads W_r once, into LDS when d·dr·4 bytes fit beside the staged rows (30 KB),
 *   through the cache otherwise; an empty relation gets no workgroup.
 *   rel_enable: uint8 [n_rel] or NULL, the `relations` argument of update_attention: v of a
 *   disabled relation's triples is not written.
 *   v: fp32 [B] in the batch's order. B = 0 launches nothing.
 *
 * hgd_kg_attention_softmax — Equation 5, torch.sparse.softmax(A_in.cpu(), dim=1) (KHGRec.py:326-
 * 331) over the UNCOALESCED batch at its fixed size: the entries of the [n_rows, n_rows] matrix
 * stay B, sorted by (row, column), and torch's coalesce-then-softmax becomes
 *   val[p] = exp(s − m)/Z for the first entry of a run of equal (row, column), s = the run's sum
 *            of v taken in the run's order, m and Z the row's max and Σ exp(s − m) over its runs;
 *   val[p] = 0 for the run's other entries — the same linear map as the coalesced matrix.
 *   rowptr: int64 [n_rows+1] and col: int32 [B], the sorted entries as a CSR; perm: int32 [B],
 *   entry p is triple perm[p] (v is read through it). rowptr[n_rows] may be below B: the entries
 *   past it (triples of disabled relations, sorted behind the last row) get val = 0. A row
 *   without entries is an empty row; nothing is written for it.
 *   A workgroup owns 256 rows: a row of up to 8 entries is done by one lane, up to 512 by a
 *   wave, a longer one by the whole workgroup (a row may be the whole batch), so a long row
 *   does not serialise on one lane. The limit of that: a RUN's sum is taken in order by the one
 *   worker that owns the run's first entry, so a row whose entries all repeat one (row, column)
 *   — up to the whole batch — is summed by a single lane, whichever form takes the row.
 *   Workspace: hgd_kg_attention_softmax_workspace_size (the runs' sums and exponentials, so that
 *   val is written once). Stream-ordered, no host synchronisation. */
hgd_status hgd_kg_attention_scores(const float* E, int64_t ldE, int64_t n_ent, const float* W,
                                   const float* R, int64_t ldR, int32_t n_rel, int32_t d,
                                   int32_t dr, const int32_t* h, const int32_t* t,
                                   const int32_t* grp_perm, const int64_t* rel_off,
                                   const uint8_t* rel_enable, int64_t B, float* v, void* stream);
size_t hgd_kg_attention_softmax_workspace_size(int64_t B);
hgd_status hgd_kg_attention_softmax(const int64_t* rowptr, const int32_t* col,
                                    const int32_t* perm, int64_t n_rows, int64_t B,
                                    const float* v, float* val, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * KG loss: KHGRec's calculate_kg_loss (model/graph/KHGRec.py:347-365, called on every minibatch,
 * :144), the TransR loss of a batch of B triples (h, r, pos_t, neg_t), forward and backward,
 * without the [B, d, dr] gather W_r = trans_M[r] and its gradient. fp32, every sum in a fixed
 * order, no float atomics: two runs are bitwise equal. With W = W[r_i], e = R[r_i]:
 *   a_i = x_h,i·W, p_i = x_p,i·W, n_i = x_n,i·W                                   (length dr)
 *   pos_i = Σ_k (a + e − p)_k²,  neg_i = Σ_k (a + e − n)_k²
 *   loss = (1/B) Σ_i softplus(pos_i − neg_i)
 *          + reg_kg · (‖A‖_F + ‖E_r‖_F + ‖P‖_F + ‖N‖_F) / batch_size_kg
 *   A, E_r, P, N the [B, dr] matrices of a_i, e (gathered: a relation counts once per triple),
 *   p_i, n_i; the norms are not squared (util/loss_torch.py:17-21). −logsigmoid(neg − pos) is
 *   evaluated as a stable softplus (finite for any finite difference). A norm that is exactly 0
 *   contributes 0 and a 0 gradient. The mean divides by B, the regulariser by batch_size_kg
 *   (they differ on a ragged last batch).
 *
 * Row sources: x_s (s = h, p, n) is a pointer, a leading dimension lds >= d and an int32 index
 *   array is [B] or NULL: row i of kind s is x_s + (is ? is[i] : i)·lds. The table form passes
 *   the same [n_ent, d] table three times with h, pos_t, neg_t; the drop-in form passes three
 *   gathered [B, d] tensors without indices. Rows need no alignment (they are staged
 *   element-wise). Indices are not range-checked here (hgd_index_narrow does that).
 * W: [n_rel, d, dr] contiguous (trans_M); R: [n_rel, dr] rows ldR apart (relation_emb);
 *   grp_perm / rel_off: the relation-grouped order of the batch, as for hgd_kg_attention_scores
 *   (all relations take part). 1 <= n_rel <= 65535, d·dr <= 2^24, 0 < B < 2^31 / 3; B = 0 is
 *   rejected (the mean over no triples is undefined).
 *
 * hgd_kg_loss_forward — a workgroup takes 32 consecutive triples of one relation in the grouped
 *   order and reads W_r once (from LDS when d·dr·4 bytes fit beside the 24 KB of staged rows:
 *   up to 36 KB; through the cache otherwise); the loss and the four sums of squares are reduced
 *   per tile and then over the tiles in tile order by one workgroup. Written in full:
 *   proj  fp32 [3, B, dr]: a, p, n in GROUPED order (row q of a plane is triple grp_perm[q]);
 *   coef  fp32 [B]: σ(pos − neg)/B, grouped order;   norms fp32 [4]: ‖A‖, ‖E_r‖, ‖P‖, ‖N‖;
 *   loss  fp32 [1].
 *
 * hgd_kg_loss_backward — `grad` is a device scalar (∂/∂loss, as in hgd_bpr_backward); proj, coef,
 *   norms are the forward's. Each output is optional (NULL = not computed):
 *   G   fp32 [3B, d] contiguous, written in full: row s·B + i = grad · ∂loss/∂x_s,i = W_r·g_s,i
 *       in the BATCH's order (s = 0, 1, 2 for h, pos_t, neg_t). For the table form the entity
 *       gradient is S·G with the binary [n_ent, 3B] matrix "entity ← position" (hgd_sort_perm
 *       over the 3B ids, hgd_rowptr_from_sorted, hgd_spmm): pull-style, untouched rows 0.
 *   dW  fp32 [n_rel, d, dr] and dR fp32 [n_rel, dr], both or neither, written in full: for
 *       relation r the sum over r's triples of x_h ⊗ g_a + x_p ⊗ g_p + x_n ⊗ g_n and of g_e,
 *       taken per 32-triple tile in grouped order and then over r's tiles in tile order (one
 *       output element per thread); a relation without triples gets exact zeros. Duplicates of
 *       a triple are counted once each, as the reference's gather does.
 *
 * Workspace: hgd_kg_loss_workspace_size(B, n_rel, d, dr) for either call (the tiles' partial
 * sums; ⌈B/32⌉ + min(n_rel, B) tiles of (d + 1)·dr floats for dW / dR). Stream-ordered, no host
 * synchronisation, no allocation. */
size_t hgd_kg_loss_workspace_size(int64_t B, int32_t n_rel, int32_t d, int32_t dr);
hgd_status hgd_kg_loss_forward(const float* xh, int64_t ldh, const int32_t* ih, const float* xp,
                               int64_t ldp, const int32_t* ip, const float* xn, int64_t ldn,
                               const int32_t* in, const float* W, const float* R, int64_t ldR,
                               int32_t n_rel, int32_t d, int32_t dr, const int32_t* grp_perm,
                               const int64_t* rel_off, int64_t B, float reg_kg,
                               int64_t batch_size_kg, float* proj, float* coef, float* norms,
                               float* loss, void* workspace, size_t workspace_bytes,
                               void* stream);
hgd_status hgd_kg_loss_backward(const float* xh, int64_t ldh, const int32_t* ih, const float* xp,
                                int64_t ldp, const int32_t* ip, const float* xn, int64_t ldn,
                                const int32_t* in, const float* W, const float* R, int64_t ldR,
                                int32_t n_rel, int32_t d, int32_t dr, const int32_t* grp_perm,
                                const int64_t* rel_off, int64_t B, float reg_kg,
                                int64_t batch_size_kg, const float* proj, const float* coef,
                                const float* norms, const float* grad, float* G, float* dW,
                                float* dR, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * View attention: KHGRec's fusion of an item's two views, Attention.forward of
 * model/graph/KHGRec.py:466-480, called at :132 (every minibatch) and :202 (every evaluation)
 * on torch.stack([item_emb_cf, item_emb_kg], dim=1). With two views z0, z1 [n_rows, d] and
 * W1 [d, d], b1 [d], W2 [d, d] (nn.Linear.weight layout, contiguous; hidden_size == in_size):
 *   t_v = tanh(z_v·W1ᵀ + b1);  q = (t_0 − t_1)·W2ᵀ;  β0 = σ(q);  out = β0 ⊙ z0 + (1 − β0) ⊙ z1
 * (σ(q) is the softmax over the two views of w_v = t_v·W2ᵀ, view 0; it is taken from one
 * exponential of −|q| and is finite for every finite q.)
 *   dq = g ⊙ (z0 − z1) ⊙ β0(1 − β0);  h = dq·W2;  da_0 = h ⊙ (1 − t_0²);  da_1 = −h ⊙ (1 − t_1²)
 *   dz_v = β_v ⊙ g + da_v·W1;  dW2 = dqᵀ·(t_0 − t_1);  dW1 = da_0ᵀ·z0 + da_1ᵀ·z1;
 *   db1 = Σ_rows (da_0 + da_1)           (β as a returned value carries no gradient)
 * d: a multiple of 16 in [16, 128]. Every row operand (z0, z1, out, beta0, g, dz0, dz1) is a
 * pointer and a leading dimension >= d with 16-byte aligned rows (pointer % 16 == 0, ld % 4 ==
 * 0): the two halves of a stacked [n_rows, 2, d] tensor are read and written in place with
 * ld = 2d. One workgroup owns hgd_view_attention_row_block() = 32 rows; the products run as
 * split-bf16 MFMAs (error ≈ 1e-7·Σ|a·b|) with the weights' fragments in registers. A row's
 * results depend on that row alone (not on n_rows or its position); no float atomics: two runs
 * are bitwise equal. n_rows = 0 validates, launches nothing and writes nothing.
 *
 * hgd_view_attention_forward — one kernel; writes out, and beta0 (β0 [n_rows, d]) unless it is
 *   NULL (evaluation / no_grad). No [n_rows, 2, d] intermediate reaches memory.
 * hgd_view_attention_backward — one kernel recomputes t_v and writes dz0, dz1 (both or neither;
 *   NULL = not computed). dW1, db1, dW2 (all or none; contiguous [d, d], [d], [d, d], written
 *   in full): the kernel also stores dq, t_0 − t_1, da_0, da_1 to the workspace and two
 *   hgd_gemm_tn calls reduce them over the rows (split-K, slices summed in slice order).
 *   Without them no workspace is read and nothing but dz0, dz1 is stored.
 * Workspace: hgd_view_attention_workspace_size(n_rows, d, ld0, ld1) for the backward with
 *   parameter gradients (4·n_rows·d floats + hgd_gemm_tn's partials); 16-byte aligned; 0 for
 *   n_rows = 0. Every argument is checked before the first HIP call (HGD_ERR_INVALID_ARG: a
 *   width that is not fused, misaligned rows, ld < d, a required pointer NULL, a workspace too
 *   small). Stream-ordered, no host synchronisation, no allocation. */
int32_t hgd_view_attention_row_block(void);
size_t hgd_view_attention_workspace_size(int64_t n_rows, int32_t d, int64_t ld0, int64_t ld1);
hgd_status hgd_view_attention_forward(const float* z0, int64_t ld0, const float* z1, int64_t ld1,
                                      int64_t n_rows, int32_t d, const float* W1,
                                      const float* b1, const float* W2, float* out, int64_t ldo,
                                      float* beta0, int64_t ldb, void* stream);
hgd_status hgd_view_attention_backward(const float* z0, int64_t ld0, const float* z1,
                                       int64_t ld1, int64_t n_rows, int32_t d, const float* W1,
                                       const float* b1, const float* W2, const float* beta0,
                                       int64_t ldb, const float* g, int64_t ldg, float* dz0,
                                       int64_t lddz0, float* dz1, int64_t lddz1, float* dW1,
                                       float* db1, float* dW2, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CF loss: KHGRec's recommendation loss of a minibatch (model/graph/KHGRec.py:131-143 and
 * calculate_cf_loss, :341-345) with the view fusion evaluated ONLY at the batch's item rows.
 * U [n_users, d] user rows; Z0, Z1 [n_items, d] the items' two views; uid, pid, nid [batch]
 * int32 ids (assumed in range: hgd_index_narrow checks them); W1, b1, W2 the Attention's
 * parameters as for the view attention, or all three NULL for the mean of the views
 * (KHGRec.py:134). Item position p in [0, 2·batch) is INTERLEAVED: p = 2k is triple k's
 * positive, p = 2k + 1 its negative (a 32-row block holds 16 whole triples):
 *   i_p  = p even ? pid[p/2] : nid[p/2]
 *   F_p  = β0 ⊙ Z0[i_p] + (1 − β0) ⊙ Z1[i_p]   (β0 as in "View attention"; mean mode: β0 = 1/2)
 *   a_k  = U[uid[k]];   x_k = <a_k, F_2k> − <a_k, F_2k+1>
 *   loss = (1/batch) Σ_k −log(1e-5 + σ(x_k)) + reg · (‖A‖_F + ‖P‖_F + ‖N‖_F) / batch_size
 * A, P, N the gathered [batch, d] matrices (a repeated row counts once per occurrence; the norms
 * are not squared, util/loss_torch.py:17-21). The mean divides by batch, the regulariser by the
 * configured batch_size. With g = *grad and c_k = σ(x)σ(−x)/(1e-5 + σ(x)) (coef):
 *   dF_2k   = −(g/batch)·c_k·a_k + (g·reg/batch_size)·F_2k/‖P‖
 *   dF_2k+1 = +(g/batch)·c_k·a_k + (g·reg/batch_size)·F_2k+1/‖N‖
 *   da_k    = −(g/batch)·c_k·(F_2k − F_2k+1) + (g·reg/batch_size)·a_k/‖A‖
 * (a norm that is exactly 0 contributes a 0 gradient), and dZ0, dZ1, dW1, db1, dW2 follow from dF
 * by the view attention's backward at the 2·batch positions (mean mode: dZ0 = dZ1 = dF/2).
 * d: a multiple of 16 in [16, 128] with parameters, a multiple of 4 in [4, 256] in mean mode.
 * Row operands are a pointer and a leading dimension >= d with 16-byte aligned rows. Work and
 * memory are O(batch·d): F and dF stay on chip, the views are read through the ids. fp32, every
 * sum in a fixed order, no float atomics: two runs are bitwise equal, and coef[k] and the
 * gradients of triple k depend on that triple's rows and on the three norms alone.
 *
 * hgd_cf_loss_forward — one row kernel (a workgroup owns 32 positions) and a single-workgroup
 *   kernel that adds the blocks' partial sums in block order. Writes coef [batch],
 *   norms [3] = (‖A‖, ‖P‖, ‖N‖), loss [1], and beta0 [2·batch, d] unless it is NULL (no backward
 *   to follow; it must be NULL in mean mode).
 * hgd_cf_loss_backward — one row kernel. dA [batch, d] (NULL = not computed), dZ0 / dZ1
 *   [2·batch, ·] per POSITION (both or neither), dW1, db1, dW2 (all or none, written in full; the
 *   kernel then also stores six [2·batch, d] operands to the workspace and hgd_gemm_tn reduces
 *   them). The fold of dA and dZ into [n_users, d] / [n_items, d] tables — the sum over the
 *   positions of each row, in ascending position order — is the CALLER's hop (an SpMM with the
 *   binary matrix "row ← position"; the Python host uses hgd_sort_perm + hgd_spmm).
 * Workspace: hgd_cf_loss_workspace_size(batch, d, with_params): the forward needs
 *   (batch, d, 0), the backward (batch, d, 1) when parameter gradients are asked for and none
 *   otherwise; 16-byte aligned. 0 for batch <= 0 or a width outside the mode's set. Every
 *   argument is checked before the first HIP call (HGD_ERR_INVALID_ARG; HGD_ERR_WORKSPACE for a
 *   workspace that is NULL or too small). batch = 0 validates and launches nothing.
 *   Stream-ordered, no host synchronisation, no allocation. */
size_t hgd_cf_loss_workspace_size(int64_t batch, int32_t d, int32_t with_params);
hgd_status hgd_cf_loss_forward(const float* U, int64_t ldu, const int32_t* uid, int64_t n_users,
                               const float* Z0, int64_t ld0, const float* Z1, int64_t ld1,
                               const int32_t* pid, const int32_t* nid, int64_t n_items,
                               int64_t batch, int32_t d, const float* W1, const float* b1,
                               const float* W2, float reg, int64_t batch_size, float* beta0,
                               int64_t ldb, float* coef, float* norms, float* loss,
                               void* workspace, size_t workspace_bytes, void* stream);
hgd_status hgd_cf_loss_backward(const float* U, int64_t ldu, const int32_t* uid, int64_t n_users,
                                const float* Z0, int64_t ld0, const float* Z1, int64_t ld1,
                                const int32_t* pid, const int32_t* nid, int64_t n_items,
                                int64_t batch, int32_t d, const float* W1, const float* b1,
                                const float* W2, float reg, int64_t batch_size,
                                const float* beta0, int64_t ldb, const float* coef,
                                const float* norms, const float* grad, float* dA, int64_t ldda,
                                float* dZ0, int64_t lddz0, float* dZ1, int64_t lddz1, float* dW1,
                                float* db1, float* dW2, void* workspace, size_t workspace_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HGD_H */
