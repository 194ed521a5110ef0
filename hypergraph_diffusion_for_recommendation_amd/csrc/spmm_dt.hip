// The SpMM hop of spmm.hip over 16-bit tables: hgd_spmm_dt / hgd_spmm_masked_dt /
// hgd_spmm_blocked_dt, and the fused row epilogue over a bfloat16 table: hgd_spmm_fused_dt /
// hgd_spmm_masked_fused_dt; and the ordered twin of each but the blocked one (hgd_spmm_ordered_dt,
// hgd_spmm_masked_ordered_dt, hgd_spmm_fused_ordered_dt, hgd_spmm_masked_fused_ordered_dt).
//
// Replaces the same call sites as hgd_spmm (torch.sparse.mm(adj, X), model/graph/HCCF.py:199;
// torch.sparse.mm(adj.t(), X), model/graph/HGNN_HD4.py:459-462, HGCN.py:173-175; paths relative
// to the reference's HD_SELFRec tree) when the embedding table is stored or staged in bfloat16.
//
// The kernels are spmm_kernels.h's, instantiated for the element types (TX of the gathered table,
// TY of the output) ∈ {bf16→bf16, bf16→f32, f32→bf16}; f32→f32 forwards to hgd_spmm. A bf16
// element is widened to fp32 exactly, the sum is the same single fp32 fmaf chain in edge order,
// weights / row scales / split-row partials / the activation are fp32, and the one new rounding
// is the bf16 store (round to nearest even).
//
// Work mapping on the aligned path: a lane owns 8 contiguous columns — one 16-byte load of a bf16
// row (two of an fp32 one) — so a group is G = d/8 lanes (d = 64: 8 lanes, 8 rows per wave) and a
// wave keeps the same U × 16 B × 64 lanes = 8 KB of gathers in flight as the fp32 hop. Rows wider
// than 128 columns run as 128-column passes (256 B of a bf16 row per gathered piece, the size of
// the fp32 hop's 64-column piece; HGD_TUNE_SPMM_PASS_COLS overrides it). Only the default cache
// policy and U = 8 are instantiated here: the d = 64 tuning matrix stays fp32-only.
//
// The checks, the pass plan and the launches are the shared launcher's (spmm_launch.h), where
// every difference from the fp32 hop is an explicit condition on the element types; this file is
// the dtype-code dispatch onto its three mixed instantiations.
#include "spmm_launch.h"

namespace hgd {
namespace {

hgd_status spmm_dt_dispatch(const SpmmRequest& r, int32_t x_dtype, int32_t y_dtype) {
  const bool xb = x_dtype == HGD_DT_BF16, yb = y_dtype == HGD_DT_BF16;
  if (xb && yb) return spmm_launch<bf16, bf16>(r);
  if (xb) return spmm_launch<bf16, float>(r);
  return spmm_launch<float, bf16>(r);
}

bool dtype_ok(int32_t dt) { return dt == HGD_DT_F32 || dt == HGD_DT_BF16; }

}  // namespace
}  // namespace hgd

extern "C" hgd_status hgd_spmm_dt(const int64_t* rowptr, const int32_t* col, const float* val,
                                  const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                                  int64_t row_begin, int64_t row_end, const void* X,
                                  int32_t x_dtype, int64_t ldx, void* Y, int32_t y_dtype,
                                  int64_t ldy, int32_t d, int32_t epilogue, float slope,
                                  const hgd_split_plan* plan, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype) && hgd::dtype_ok(y_dtype),
              "hgd_spmm_dt: unknown dtype code (x %d, y %d): HGD_DT_F32 or HGD_DT_BF16", x_dtype,
              y_dtype);
  if (x_dtype == HGD_DT_F32 && y_dtype == HGD_DT_F32)
    return hgd_spmm(rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin, row_end,
                    static_cast<const float*>(X), ldx, static_cast<float*>(Y), ldy, d, epilogue,
                    slope, plan, workspace, workspace_bytes, stream);
  hgd::SpmmRequest r{"hgd_spmm_dt", rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                     row_end, X, ldx, Y, ldy, d, epilogue, slope, plan, workspace, workspace_bytes,
                     stream};
  return hgd::spmm_dt_dispatch(r, x_dtype, y_dtype);
}

extern "C" hgd_status hgd_spmm_masked_dt(const int64_t* rowptr, const int32_t* col,
                                         const float* val, const uint8_t* mask, float keep,
                                         const float* row_scale, int64_t n_rows,
                                         int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                                         const void* X, int32_t x_dtype, int64_t ldx, void* Y,
                                         int32_t y_dtype, int64_t ldy, int32_t d,
                                         int32_t epilogue, float slope,
                                         const hgd_split_plan* plan, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype) && hgd::dtype_ok(y_dtype),
              "hgd_spmm_masked_dt: unknown dtype code (x %d, y %d): HGD_DT_F32 or HGD_DT_BF16",
              x_dtype, y_dtype);
  if (x_dtype == HGD_DT_F32 && y_dtype == HGD_DT_F32)
    return hgd_spmm_masked(rowptr, col, val, mask, keep, row_scale, n_rows, n_src_rows, row_begin,
                           row_end, static_cast<const float*>(X), ldx, static_cast<float*>(Y),
                           ldy, d, epilogue, slope, plan, workspace, workspace_bytes, stream);
  hgd::SpmmRequest r{"hgd_spmm_masked_dt", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, epilogue, slope, plan, workspace,
                     workspace_bytes, stream};
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  return hgd::spmm_dt_dispatch(r, x_dtype, y_dtype);
}

// The fused row epilogue (hgd_spmm_fused / hgd_spmm_masked_fused; HGCNConv + LayerNorm + residual,
// model/layers/EquivSetConv.py:86-107, model/graph/HGNN_HD3.py:705-720; HCCF's layer,
// model/graph/HCCF.py:182-187) over a bfloat16 table: the bf16→f32 instantiation of the EX row
// kernel, its masked form and the EX fix-up of split rows. Y, the side tables, the LayerNorm
// statistics and the split-row partials are fp32; y16 (or NULL) receives the row of Y rounded to
// bf16 from the same registers, which the next layer's first hop gathers.
namespace hgd {
namespace {

hgd_status spmm_fused_dt(SpmmRequest r, const hgd_row_epilogue* epi, void* y16, int64_t ld_y16) {
  HGD_REQUIRE(epi != nullptr, "%s: null epilogue descriptor", r.fn);
  r.epilogue = epi->act;
  r.slope = epi->slope;
  r.ex = epi;
  r.y16 = y16;
  r.ld_y16 = ld_y16;
  return spmm_launch<bf16, float>(r);
}

}  // namespace
}  // namespace hgd

extern "C" hgd_status hgd_spmm_fused_dt(const int64_t* rowptr, const int32_t* col,
                                        const float* val, const float* row_scale, int64_t n_rows,
                                        int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                                        const void* X, int32_t x_dtype, int64_t ldx, float* Y,
                                        int64_t ldy, int32_t d, const hgd_row_epilogue* epi,
                                        void* y16, int64_t ld_y16, const hgd_split_plan* plan,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype),
              "hgd_spmm_fused_dt: unknown dtype code (x %d): HGD_DT_F32 or HGD_DT_BF16", x_dtype);
  if (x_dtype == HGD_DT_F32) {
    if (y16)
      return hgd::fail(HGD_ERR_UNSUPPORTED,
                       "hgd_spmm_fused_dt: y16 needs a bfloat16 table (x HGD_DT_F32)");
    return hgd_spmm_fused(rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin, row_end,
                          static_cast<const float*>(X), ldx, Y, ldy, d, epi, plan, workspace,
                          workspace_bytes, stream);
  }
  hgd::SpmmRequest r{"hgd_spmm_fused_dt", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, HGD_EPI_NONE, 0.f, plan, workspace,
                     workspace_bytes, stream};
  return hgd::spmm_fused_dt(r, epi, y16, ld_y16);
}

extern "C" hgd_status hgd_spmm_masked_fused_dt(const int64_t* rowptr, const int32_t* col,
                                               const float* val, const uint8_t* mask, float keep,
                                               const float* row_scale, int64_t n_rows,
                                               int64_t n_src_rows, int64_t row_begin,
                                               int64_t row_end, const void* X, int32_t x_dtype,
                                               int64_t ldx, float* Y, int64_t ldy, int32_t d,
                                               const hgd_row_epilogue* epi, void* y16,
                                               int64_t ld_y16, const hgd_split_plan* plan,
                                               void* workspace, size_t workspace_bytes,
                                               void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype),
              "hgd_spmm_masked_fused_dt: unknown dtype code (x %d): HGD_DT_F32 or HGD_DT_BF16",
              x_dtype);
  if (x_dtype == HGD_DT_F32) {
    if (y16)
      return hgd::fail(HGD_ERR_UNSUPPORTED,
                       "hgd_spmm_masked_fused_dt: y16 needs a bfloat16 table (x HGD_DT_F32)");
    return hgd_spmm_masked_fused(rowptr, col, val, mask, keep, row_scale, n_rows, n_src_rows,
                                 row_begin, row_end, static_cast<const float*>(X), ldx, Y, ldy, d,
                                 epi, plan, workspace, workspace_bytes, stream);
  }
  hgd::SpmmRequest r{"hgd_spmm_masked_fused_dt", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, HGD_EPI_NONE, 0.f, plan, workspace,
                     workspace_bytes, stream};
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  return hgd::spmm_fused_dt(r, epi, y16, ld_y16);
}

// The source-blocked hop (hgd_spmm_blocked) over 16-bit tables: the launcher's block loop over the
// same three instantiations. An fp32 Y carries its own running partial, as in the fp32 hop; a
// bf16 Y keeps it in the caller's fp32 scratch and is stored once, after the last block, so it is
// the fp32 result of the same call rounded once.
extern "C" size_t hgd_spmm_blocked_dt_workspace_size(int64_t n_rows, int32_t d, int32_t y_dtype,
                                                     int32_t n_blocks) {
  return hgd::blocked_part_bytes(n_rows, d, y_dtype == HGD_DT_BF16 ? 2 : 4, n_blocks);
}

extern "C" hgd_status hgd_spmm_blocked_dt(const int64_t* blk_start, const int32_t* blk_col,
                                          const float* blk_val, const float* row_scale,
                                          int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                          int64_t row_end, const void* X, int32_t x_dtype,
                                          int64_t ldx, void* Y, int32_t y_dtype, int64_t ldy,
                                          int32_t d, int32_t epilogue, float slope,
                                          int32_t n_blocks, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype) && hgd::dtype_ok(y_dtype),
              "hgd_spmm_blocked_dt: unknown dtype code (x %d, y %d): HGD_DT_F32 or HGD_DT_BF16",
              x_dtype, y_dtype);
  if (x_dtype == HGD_DT_F32 && y_dtype == HGD_DT_F32)
    return hgd_spmm_blocked(blk_start, blk_col, blk_val, row_scale, n_rows, n_src_rows, row_begin,
                            row_end, static_cast<const float*>(X), ldx, static_cast<float*>(Y),
                            ldy, d, epilogue, slope, n_blocks, stream);
  hgd::SpmmRequest r{"hgd_spmm_blocked_dt", nullptr, blk_col, blk_val, row_scale, n_rows,
                     n_src_rows, row_begin, row_end, X, ldx, Y, ldy, d, epilogue, slope};
  r.blocked = true;
  r.blk_start = blk_start;
  r.n_blk = n_blocks;
  r.workspace = workspace;
  r.workspace_bytes = workspace_bytes;
  r.stream = stream;
  return hgd::spmm_dt_dispatch(r, x_dtype, y_dtype);
}

extern "C" int32_t hgd_spmm_blocks_for_dt(int64_t n_src_rows, int32_t d, int32_t x_dtype) {
  if (x_dtype == HGD_DT_F32) return hgd_spmm_blocks_for(n_src_rows, d);
  // 16-bit tables: never by size. Measured on MI355X at 10 M users × 1 M items × 100 M edges
  // (scripts/bench_mall_blocked.py --table-dtype bf16, profiles/bf16_blocked/):
  // no block count beat the plain bf16 hop into items at any size tried — the 1.28 GB table at
  // d = 64: 2.830 ms plain, 2.881 at P = 2, 3.454 at P = 8; the 2.56 GB table at d = 128: 5.648 /
  // 5.856 / 7.274; d = 256 in 128-column passes: 11.39 / 11.74 / 14.57 — against a round-to-round
  // spread of 0.01–0.03 ms. The hop is reachable through HGD_SPMM_BLOCKS=P in the Python host.
  return 0;
}

// The ordered twins of hgd_spmm_dt / hgd_spmm_masked_dt / hgd_spmm_fused_dt /
// hgd_spmm_masked_fused_dt (hgd_spmm_ordered's contract: rowptr / col / val / row_scale the
// ordered copies, out_row the order, every row; mask in the ordered entry order; what epi points
// to and y16 indexed by Y row). f32 → f32 forwards to the fp32 ordered twin, as the unordered
// entry points forward to theirs.
extern "C" hgd_status hgd_spmm_ordered_dt(const int64_t* rowptr, const int32_t* col,
                                          const float* val, const float* row_scale,
                                          int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                          int64_t row_end, const void* X, int32_t x_dtype,
                                          int64_t ldx, void* Y, int32_t y_dtype, int64_t ldy,
                                          int32_t d, int32_t epilogue, float slope,
                                          const hgd_split_plan* plan, void* workspace,
                                          size_t workspace_bytes, const int32_t* out_row,
                                          void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype) && hgd::dtype_ok(y_dtype),
              "hgd_spmm_ordered_dt: unknown dtype code (x %d, y %d): HGD_DT_F32 or HGD_DT_BF16",
              x_dtype, y_dtype);
  if (x_dtype == HGD_DT_F32 && y_dtype == HGD_DT_F32)
    return hgd_spmm_ordered(rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin, row_end,
                            static_cast<const float*>(X), ldx, static_cast<float*>(Y), ldy, d,
                            epilogue, slope, plan, workspace, workspace_bytes, out_row, stream);
  hgd::SpmmRequest r{"hgd_spmm_ordered_dt", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, epilogue, slope, plan, workspace,
                     workspace_bytes, stream};
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_dt_dispatch(r, x_dtype, y_dtype);
}

extern "C" hgd_status hgd_spmm_masked_ordered_dt(const int64_t* rowptr, const int32_t* col,
                                                 const float* val, const uint8_t* mask, float keep,
                                                 const float* row_scale, int64_t n_rows,
                                                 int64_t n_src_rows, int64_t row_begin,
                                                 int64_t row_end, const void* X, int32_t x_dtype,
                                                 int64_t ldx, void* Y, int32_t y_dtype,
                                                 int64_t ldy, int32_t d, int32_t epilogue,
                                                 float slope, const hgd_split_plan* plan,
                                                 void* workspace, size_t workspace_bytes,
                                                 const int32_t* out_row, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype) && hgd::dtype_ok(y_dtype),
              "hgd_spmm_masked_ordered_dt: unknown dtype code (x %d, y %d): HGD_DT_F32 or "
              "HGD_DT_BF16", x_dtype, y_dtype);
  if (x_dtype == HGD_DT_F32 && y_dtype == HGD_DT_F32)
    return hgd_spmm_masked_ordered(rowptr, col, val, mask, keep, row_scale, n_rows, n_src_rows,
                                   row_begin, row_end, static_cast<const float*>(X), ldx,
                                   static_cast<float*>(Y), ldy, d, epilogue, slope, plan,
                                   workspace, workspace_bytes, out_row, stream);
  hgd::SpmmRequest r{"hgd_spmm_masked_ordered_dt", rowptr, col, val, row_scale, n_rows,
                     n_src_rows, row_begin, row_end, X, ldx, Y, ldy, d, epilogue, slope, plan,
                     workspace, workspace_bytes, stream};
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_dt_dispatch(r, x_dtype, y_dtype);
}

extern "C" hgd_status hgd_spmm_fused_ordered_dt(const int64_t* rowptr, const int32_t* col,
                                                const float* val, const float* row_scale,
                                                int64_t n_rows, int64_t n_src_rows,
                                                int64_t row_begin, int64_t row_end, const void* X,
                                                int32_t x_dtype, int64_t ldx, float* Y,
                                                int64_t ldy, int32_t d,
                                                const hgd_row_epilogue* epi, void* y16,
                                                int64_t ld_y16, const hgd_split_plan* plan,
                                                void* workspace, size_t workspace_bytes,
                                                const int32_t* out_row, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype),
              "hgd_spmm_fused_ordered_dt: unknown dtype code (x %d): HGD_DT_F32 or HGD_DT_BF16",
              x_dtype);
  if (x_dtype == HGD_DT_F32) {
    if (y16)
      return hgd::fail(HGD_ERR_UNSUPPORTED,
                       "hgd_spmm_fused_ordered_dt: y16 needs a bfloat16 table (x HGD_DT_F32)");
    return hgd_spmm_fused_ordered(rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                                  row_end, static_cast<const float*>(X), ldx, Y, ldy, d, epi,
                                  plan, workspace, workspace_bytes, out_row, stream);
  }
  hgd::SpmmRequest r{"hgd_spmm_fused_ordered_dt", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, HGD_EPI_NONE, 0.f, plan, workspace,
                     workspace_bytes, stream};
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_fused_dt(r, epi, y16, ld_y16);
}

extern "C" hgd_status hgd_spmm_masked_fused_ordered_dt(
    const int64_t* rowptr, const int32_t* col, const float* val, const uint8_t* mask, float keep,
    const float* row_scale, int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
    int64_t row_end, const void* X, int32_t x_dtype, int64_t ldx, float* Y, int64_t ldy,
    int32_t d, const hgd_row_epilogue* epi, void* y16, int64_t ld_y16,
    const hgd_split_plan* plan, void* workspace, size_t workspace_bytes, const int32_t* out_row,
    void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(hgd::dtype_ok(x_dtype),
              "hgd_spmm_masked_fused_ordered_dt: unknown dtype code (x %d): HGD_DT_F32 or "
              "HGD_DT_BF16", x_dtype);
  if (x_dtype == HGD_DT_F32) {
    if (y16)
      return hgd::fail(HGD_ERR_UNSUPPORTED, "hgd_spmm_masked_fused_ordered_dt: y16 needs a "
                       "bfloat16 table (x HGD_DT_F32)");
    return hgd_spmm_masked_fused_ordered(rowptr, col, val, mask, keep, row_scale, n_rows,
                                         n_src_rows, row_begin, row_end,
                                         static_cast<const float*>(X), ldx, Y, ldy, d, epi, plan,
                                         workspace, workspace_bytes, out_row, stream);
  }
  hgd::SpmmRequest r{"hgd_spmm_masked_fused_ordered_dt", rowptr, col, val, row_scale, n_rows,
                     n_src_rows, row_begin, row_end, X, ldx, Y, ldy, d, HGD_EPI_NONE, 0.f, plan,
                     workspace, workspace_bytes, stream};
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_fused_dt(r, epi, y16, ld_y16);
}
