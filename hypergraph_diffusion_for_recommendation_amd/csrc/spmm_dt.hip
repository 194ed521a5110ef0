// The SpMM hop of spmm.hip over 16-bit tables: hgd_spmm_dt / hgd_spmm_masked_dt.
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
#include <cmath>

#include "spmm_kernels.h"

namespace hgd {
namespace {

constexpr int kU = 8;
constexpr int kPol = kPolPrefetch;

template <int G, int VEC, class TX, class TY>
void launch_rows(const SpmmArgsT<TX, TY>& a, bool has_val, bool seg, int64_t blocks,
                 hipStream_t st) {
  if (a.mask) {  // masked (edge-dropped view) hop: the row kernel only
    if (has_val)
      hipLaunchKernelGGL((spmm_kernel<G, VEC, kU, true, kPol, false, true, TX, TY>), dim3(blocks),
                         dim3(kBlock), 0, st, a);
    else
      hipLaunchKernelGGL((spmm_kernel<G, VEC, kU, false, kPol, false, true, TX, TY>), dim3(blocks),
                         dim3(kBlock), 0, st, a);
    return;
  }
  if constexpr (G >= 8) {
    if (seg) {
      if (has_val)
        hipLaunchKernelGGL((spmm_seg_kernel<G, VEC, kU, true, kPol, false, TX, TY>), dim3(blocks),
                           dim3(kBlock), 0, st, a);
      else
        hipLaunchKernelGGL((spmm_seg_kernel<G, VEC, kU, false, kPol, false, TX, TY>),
                           dim3(blocks), dim3(kBlock), 0, st, a);
      return;
    }
  }
  if (has_val)
    hipLaunchKernelGGL((spmm_kernel<G, VEC, kU, true, kPol, false, false, TX, TY>), dim3(blocks),
                       dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((spmm_kernel<G, VEC, kU, false, kPol, false, false, TX, TY>), dim3(blocks),
                       dim3(kBlock), 0, st, a);
}

// One column pass: the segmented walk, or the row kernel (split-row chunks first in the grid) and
// the fix-up of the split rows — the launch shapes of spmm.hip's launch_g.
template <int G, int VEC, class TX, class TY>
hgd_status launch_g(SpmmArgsT<TX, TY> a, bool has_val, hipStream_t st) {
  constexpr int GPB = kBlock / G;
  const int64_t rows = a.row_end - a.row_begin;
  if constexpr (G >= 8) {
    if (a.seg) {
      const int64_t sblocks = (rows + static_cast<int64_t>(GPB) * G - 1) / (GPB * G);
      if (sblocks <= 0) return HGD_OK;
      if (sblocks > 0x7fffffffLL) return fail(HGD_ERR_UNSUPPORTED, "hgd_spmm_dt: grid too large");
      launch_rows<G, VEC>(a, has_val, true, sblocks, st);
      return check_launch("hgd_spmm_dt segmented kernel");
    }
  }
  a.heavy_blocks = (a.n_chunks + GPB - 1) / GPB;
  const int64_t blocks = (rows + GPB - 1) / GPB + a.heavy_blocks;
  if (blocks > 0) {
    if (blocks > 0x7fffffffLL) return fail(HGD_ERR_UNSUPPORTED, "hgd_spmm_dt: grid too large");
    launch_rows<G, VEC>(a, has_val, false, blocks, st);
    hgd_status s = check_launch("hgd_spmm_dt kernel");
    if (s != HGD_OK) return s;
  }
  if (a.n_heavy > 0) {
    if (a.n_heavy > 0x7fffffffLL)
      return fail(HGD_ERR_UNSUPPORTED, "hgd_spmm_dt: too many split rows");
    hipLaunchKernelGGL((spmm_fixup_kernel<G, VEC, false, TX, TY>), dim3(a.n_heavy), dim3(kBlock),
                       0, st, a);
    return check_launch("hgd_spmm_dt fixup");
  }
  return HGD_OK;
}

template <int VEC, class TX, class TY>
hgd_status launch_vec(int G, const SpmmArgsT<TX, TY>& a, bool has_val, hipStream_t st) {
  switch (G) {
    case 1: return launch_g<1, VEC>(a, has_val, st);
    case 2: return launch_g<2, VEC>(a, has_val, st);
    case 4: return launch_g<4, VEC>(a, has_val, st);
    case 8: return launch_g<8, VEC>(a, has_val, st);
    case 16: return launch_g<16, VEC>(a, has_val, st);
    case 32: return launch_g<32, VEC>(a, has_val, st);
    case 64:  // a pass of the 8-column path is at most 256 columns: 32 lanes
      if constexpr (VEC == 1) return launch_g<64, VEC>(a, has_val, st);
      [[fallthrough]];
    default: return fail(HGD_ERR_UNSUPPORTED, "hgd_spmm_dt: unsupported group size %d", G);
  }
}

template <class T>
constexpr int64_t kVecElems = 16 / static_cast<int64_t>(sizeof(T));  // elements per 16 bytes

template <class TX, class TY>
hgd_status spmm_dt_impl(const int64_t* rowptr, const int32_t* col, const float* val,
                        const float* row_scale, int64_t row_begin, int64_t row_end, const TX* X,
                        int64_t ldx, TY* Y, int64_t ldy, int32_t d, int32_t epilogue, float slope,
                        const uint8_t* mask, float keep, const hgd_split_plan* plan,
                        void* workspace, size_t workspace_bytes, void* stream, const char* fn) {
  SpmmArgsT<TX, TY> a{};
  a.rowptr = rowptr;
  a.col = col;
  a.val = val;
  a.row_scale = row_scale;
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.X = X;
  a.ldx = ldx;
  a.Y = Y;
  a.ldy = ldy;
  a.d = d;
  a.epi = epilogue;
  a.slope = slope;
  a.mask = mask;
  a.keep = keep;
  {
    int e2 = 0;
    a.inv_keep = (!g_mask_div && keep > 0.f && std::frexp(keep, &e2) == 0.5f) ? 1.f / keep : 0.f;
  }
  a.mask_pair = g_mask_pair;
  if (plan && plan->threshold > 0 && plan->n_heavy > 0) {
    HGD_REQUIRE(plan->chunk > 0 && plan->heavy_rows && plan->heavy_cptr && plan->chunk_heavy,
                "%s: incomplete split plan", fn);
    const size_t need = hgd_spmm_workspace_size(plan, d);  // fp32 partials, as hgd_spmm's
    if (workspace_bytes < need || (need && !workspace))
      return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", fn, workspace_bytes,
                  need);
    a.heavy_threshold = plan->threshold;
    a.chunk = plan->chunk;
    a.n_chunks = plan->n_chunks;
    a.n_heavy = plan->n_heavy;
    a.chunk_heavy = plan->chunk_heavy;
    a.heavy_rows = plan->heavy_rows;
    a.heavy_cptr = plan->heavy_cptr;
    a.partial = static_cast<float*>(workspace);
  } else if (plan && (plan->flags & HGD_PLAN_SEGMENTED) && !mask) {
    a.seg = 1;  // only without split rows: the segmented walk covers every nonzero of its rows
  }

  hipStream_t st = as_stream(stream);
  const bool has_val = val != nullptr;
  // 16-byte rows: a lane's 8 columns are one access of a bf16 row, two of an fp32 row
  auto al16 = [](const void* p, int64_t ld, int64_t per16) {
    return p == nullptr || (reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % per16 == 0);
  };
  const bool aligned = d % 8 == 0 && al16(X, ldx, kVecElems<TX>) && al16(Y, ldy, kVecElems<TY>);
  if (aligned) {
    const int lanes = d / 8;
    int G = lanes >= 64 ? 64 : next_pow2(lanes);
    const int tuned = spmm_pass_cols();
    const int pass_cols = tuned ? tuned : 128;
    if (8 * G > pass_cols) G = pass_cols / 8;
    for (int c0 = 0; c0 < d; c0 += 8 * G) {
      a.col0 = c0;
      hgd_status s = launch_vec<8>(G, a, has_val, st);
      if (s != HGD_OK) return s;
    }
  } else {
    const int G = d >= 64 ? 64 : next_pow2(d);
    for (int c0 = 0; c0 < d; c0 += G) {
      a.col0 = c0;
      hgd_status s = launch_vec<1>(G, a, has_val, st);
      if (s != HGD_OK) return s;
    }
  }
  return HGD_OK;
}

hgd_status spmm_dt_dispatch(const int64_t* rowptr, const int32_t* col, const float* val,
                            const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                            int64_t row_begin, int64_t row_end, const void* X, int32_t x_dtype,
                            int64_t ldx, void* Y, int32_t y_dtype, int64_t ldy, int32_t d,
                            int32_t epilogue, float slope, const uint8_t* mask, float keep,
                            const hgd_split_plan* plan, void* workspace, size_t workspace_bytes,
                            void* stream, const char* fn) {
  HGD_REQUIRE(d > 0, "%s: d must be > 0 (got %d)", fn, d);
  HGD_REQUIRE(n_rows >= 0 && n_src_rows >= 0, "%s: negative sizes", fn);
  HGD_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n_rows,
              "%s: row range [%lld,%lld) outside [0,%lld)", fn, (long long)row_begin,
              (long long)row_end, (long long)n_rows);
  HGD_REQUIRE(ldx >= d && ldy >= d, "%s: ldx/ldy must be >= d", fn);
  HGD_REQUIRE(epilogue >= HGD_EPI_NONE && epilogue <= HGD_EPI_RELU, "%s: bad epilogue %d", fn,
              epilogue);
  if (row_end == row_begin) return HGD_OK;
  // col / X may be NULL for a structure without nonzeros (never dereferenced then).
  HGD_REQUIRE(rowptr && Y, "%s: null rowptr/Y", fn);
  HGD_REQUIRE(X || n_src_rows == 0, "%s: null X", fn);
  const bool xb = x_dtype == HGD_DT_BF16, yb = y_dtype == HGD_DT_BF16;
  if (xb && yb)
    return spmm_dt_impl(rowptr, col, val, row_scale, row_begin, row_end,
                        static_cast<const bf16*>(X), ldx, static_cast<bf16*>(Y), ldy, d, epilogue,
                        slope, mask, keep, plan, workspace, workspace_bytes, stream, fn);
  if (xb)
    return spmm_dt_impl(rowptr, col, val, row_scale, row_begin, row_end,
                        static_cast<const bf16*>(X), ldx, static_cast<float*>(Y), ldy, d, epilogue,
                        slope, mask, keep, plan, workspace, workspace_bytes, stream, fn);
  return spmm_dt_impl(rowptr, col, val, row_scale, row_begin, row_end,
                      static_cast<const float*>(X), ldx, static_cast<bf16*>(Y), ldy, d, epilogue,
                      slope, mask, keep, plan, workspace, workspace_bytes, stream, fn);
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
  return hgd::spmm_dt_dispatch(rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                               row_end, X, x_dtype, ldx, Y, y_dtype, ldy, d, epilogue, slope,
                               nullptr, 1.f, plan, workspace, workspace_bytes, stream,
                               "hgd_spmm_dt");
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
  HGD_REQUIRE(keep > 0.f, "hgd_spmm_masked_dt: keep must be > 0 (got %g)", (double)keep);
  HGD_REQUIRE(mask || row_end == row_begin, "hgd_spmm_masked_dt: null mask");
  return hgd::spmm_dt_dispatch(rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                               row_end, X, x_dtype, ldx, Y, y_dtype, ldy, d, epilogue, slope, mask,
                               keep, plan, workspace, workspace_bytes, stream,
                               "hgd_spmm_masked_dt");
}
