// Host side of the CSR row-gather SpMM hop, shared by spmm.hip (f32→f32) and spmm_dt.hip (a 16-bit
// table and / or output): the argument checks, the SpmmArgsT fill, the pass plan and the launch
// chain down to the kernels of spmm_kernels.h, templated on the element types (TX of the gathered
// table, TY of the output) where the kernels are. What only one of the two does is an explicit
// `if constexpr (kF32<TX, TY>)` here. Not part of the ABI.
#pragma once

#include <cmath>
#include <type_traits>

#include "spmm_kernels.h"

namespace hgd {

constexpr int kDefaultPolicy = kPolPrefetch;
static_assert(SpmmTuning{}.policy == kDefaultPolicy && SpmmTuning{}.unroll == 8);

template <class TX, class TY>
constexpr bool kF32 = std::is_same_v<TX, float> && std::is_same_v<TY, float>;

// What a launch needs besides the argument block; fn is the entry point the caller called.
struct SpmmLaunch {
  const char* fn;
  bool has_val;
  hipStream_t st;
};

inline hgd_status check_launch(const char* fn, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HGD_ERR_HIP, "%s %s: %s", fn, what, hipGetErrorString(e));
  return HGD_OK;
}

template <int G, int VEC, int U, int POL, bool EX, class TX, class TY>
void launch_kernel(const SpmmArgsT<TX, TY>& a, const SpmmLaunch& L, bool seg, int64_t blocks) {
  if constexpr (POL == kDefaultPolicy && U == 8) {
    if (a.mask) {  // masked (edge-dropped view) hop: the row kernel only
      if (L.has_val)
        hipLaunchKernelGGL((spmm_kernel<G, VEC, U, true, POL, EX, true, TX, TY>), dim3(blocks),
                           dim3(kBlock), 0, L.st, a);
      else
        hipLaunchKernelGGL((spmm_kernel<G, VEC, U, false, POL, EX, true, TX, TY>), dim3(blocks),
                           dim3(kBlock), 0, L.st, a);
      return;
    }
  }
  if constexpr (G >= 8) {
    if (seg) {
      if (L.has_val)
        hipLaunchKernelGGL((spmm_seg_kernel<G, VEC, U, true, POL, EX, TX, TY>), dim3(blocks),
                           dim3(kBlock), 0, L.st, a);
      else
        hipLaunchKernelGGL((spmm_seg_kernel<G, VEC, U, false, POL, EX, TX, TY>), dim3(blocks),
                           dim3(kBlock), 0, L.st, a);
      return;
    }
  }
  if constexpr (kF32<TX, TY> && !EX) {
    if (a.out_row) {  // the ordered hop (no mask, no segmented walk: spmm_launch)
      if (L.has_val)
        hipLaunchKernelGGL((spmm_kernel<G, VEC, U, true, POL, false, false, TX, TY, true>),
                           dim3(blocks), dim3(kBlock), 0, L.st, a);
      else
        hipLaunchKernelGGL((spmm_kernel<G, VEC, U, false, POL, false, false, TX, TY, true>),
                           dim3(blocks), dim3(kBlock), 0, L.st, a);
      return;
    }
  }
  if (L.has_val)
    hipLaunchKernelGGL((spmm_kernel<G, VEC, U, true, POL, EX, false, TX, TY>), dim3(blocks),
                       dim3(kBlock), 0, L.st, a);
  else
    hipLaunchKernelGGL((spmm_kernel<G, VEC, U, false, POL, EX, false, TX, TY>), dim3(blocks),
                       dim3(kBlock), 0, L.st, a);
}

template <int G, int VEC, bool EX, class TX, class TY>
void launch_tuned(const SpmmArgsT<TX, TY>& a, const SpmmLaunch& L, bool seg, int64_t blocks) {
  if constexpr (kF32<TX, TY> && G == 16 && VEC == 4 && !EX) {
    // the fp32 d = 64 path without a mask carries the tuning matrix (unroll × {plain, nt-store,
    // prefetch, both, prefetch + nt-index, prefetch + nt-index + nt-store})
    if (!a.mask) {
      const SpmmTuning& t = spmm_tuning();
#define HGD_POL_CASES(U)                                                                  \
      switch (t.policy) {                                                                 \
        case 0: return launch_kernel<G, VEC, U, 0, false>(a, L, seg, blocks);             \
        case 1: return launch_kernel<G, VEC, U, 1, false>(a, L, seg, blocks);             \
        case 9: return launch_kernel<G, VEC, U, 9, false>(a, L, seg, blocks);             \
        case 10: return launch_kernel<G, VEC, U, 10, false>(a, L, seg, blocks);           \
        case 11: return launch_kernel<G, VEC, U, 11, false>(a, L, seg, blocks);           \
        default: return launch_kernel<G, VEC, U, 8, false>(a, L, seg, blocks);            \
      }
      if (t.unroll >= 16) { HGD_POL_CASES(16) }
      HGD_POL_CASES(8)
#undef HGD_POL_CASES
    }
  }
  // everything else (a 16-bit side, another width, the fused epilogue, the masked hop): U = 8 with
  // the prefetch policy
  launch_kernel<G, VEC, 8, kDefaultPolicy, EX>(a, L, seg, blocks);
}

// One column pass: the segmented walk, or the row kernel (split-row chunks first in the grid) and
// the fix-up of the split rows.
template <int G, int VEC, bool EX, class TX, class TY>
hgd_status launch_g(SpmmArgsT<TX, TY> a, const SpmmLaunch& L) {
  constexpr int GPB = kBlock / G;
  const int64_t rows = a.row_end - a.row_begin;
  if constexpr (G >= 8) {
    if (a.seg) {
      const int64_t sblocks = (rows + static_cast<int64_t>(GPB) * G - 1) / (GPB * G);
      if (sblocks <= 0) return HGD_OK;
      if (sblocks > 0x7fffffffLL) return fail(HGD_ERR_UNSUPPORTED, "%s: grid too large", L.fn);
      launch_tuned<G, VEC, EX>(a, L, true, sblocks);
      return check_launch(L.fn, "segmented kernel");
    }
  }
  int64_t light_blocks = (rows + GPB - 1) / GPB;
  a.heavy_blocks = (a.n_chunks + GPB - 1) / GPB;
  if (a.n_pass > 1) light_blocks = (light_blocks + 7) / 8 * 8 * a.n_pass;  // (no split rows)
  const int64_t blocks = light_blocks + a.heavy_blocks;
  if (blocks > 0) {
    if (blocks > 0x7fffffffLL) return fail(HGD_ERR_UNSUPPORTED, "%s: grid too large", L.fn);
    launch_tuned<G, VEC, EX>(a, L, false, blocks);
    hgd_status s = check_launch(L.fn, "kernel");
    if (s != HGD_OK) return s;
  }
  if (a.n_heavy > 0) {
    if (a.n_heavy > 0x7fffffffLL)
      return fail(HGD_ERR_UNSUPPORTED, "%s: too many split rows", L.fn);
    hipLaunchKernelGGL((spmm_fixup_kernel<G, VEC, EX, TX, TY>), dim3(a.n_heavy), dim3(kBlock), 0,
                       L.st, a);
    return check_launch(L.fn, "fixup");
  }
  return HGD_OK;
}

template <int VEC, bool EX, class TX, class TY>
hgd_status launch_vec(int G, const SpmmArgsT<TX, TY>& a, const SpmmLaunch& L) {
  switch (G) {
    case 1: return launch_g<1, VEC, EX>(a, L);
    case 2: return launch_g<2, VEC, EX>(a, L);
    case 4: return launch_g<4, VEC, EX>(a, L);
    case 8: return launch_g<8, VEC, EX>(a, L);
    case 16: return launch_g<16, VEC, EX>(a, L);
    case 32: return launch_g<32, VEC, EX>(a, L);
    case 64:  // a pass of the 8-column path is at most 256 columns: 32 lanes
      if constexpr (VEC != 8) return launch_g<64, VEC, EX>(a, L);
      [[fallthrough]];
    default: return fail(HGD_ERR_UNSUPPORTED, "%s: unsupported group size %d", L.fn, G);
  }
}

// The checks that do not depend on the element types. *run = false: an empty row range, nothing
// to launch (the caller returns HGD_OK).
inline hgd_status spmm_check_args(const char* fn, const void* rowptr, int64_t n_rows,
                                  int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                                  const void* X, int64_t ldx, const void* Y, int64_t ldy,
                                  int32_t d, int32_t epilogue, float slope,
                                  const hgd_row_epilogue* ex, bool* run) {
  *run = false;
  HGD_REQUIRE(d > 0, "%s: d must be > 0 (got %d)", fn, d);
  HGD_REQUIRE(n_rows >= 0 && n_src_rows >= 0, "%s: negative sizes", fn);
  HGD_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n_rows,
              "%s: row range [%lld,%lld) outside [0,%lld)", fn, (long long)row_begin,
              (long long)row_end, (long long)n_rows);
  HGD_REQUIRE(ldx >= d && ldy >= d, "%s: ldx/ldy must be >= d", fn);
  HGD_REQUIRE(epilogue >= HGD_EPI_NONE && epilogue <= HGD_EPI_RELU, "%s: bad epilogue %d", fn,
              epilogue);
  if (ex) {
    HGD_REQUIRE(epilogue == HGD_EPI_NONE || slope >= 0.f,
                "%s: a fused activation needs slope >= 0 (got %g)", fn, (double)slope);
    HGD_REQUIRE(ex->layer_norm == 0 || ex->layer_norm == 1, "%s: layer_norm must be 0/1", fn);
    HGD_REQUIRE(!ex->res1 || ex->ld_res1 >= d, "%s: ld_res1 < d", fn);
    HGD_REQUIRE(!ex->res2 || ex->ld_res2 >= d, "%s: ld_res2 < d", fn);
    HGD_REQUIRE(!ex->act_out || ex->ld_act >= d, "%s: ld_act < d", fn);
    HGD_REQUIRE((ex->sum_out == nullptr) == (ex->sum_res == nullptr),
                "%s: sum_out and sum_res go together", fn);
    HGD_REQUIRE(!ex->sum_out || (ex->ld_sum_out >= d && ex->ld_sum_res >= d),
                "%s: ld_sum_out / ld_sum_res < d", fn);
  }
  if (row_end == row_begin) return HGD_OK;
  // col / X may be NULL for a structure without nonzeros (never dereferenced then).
  HGD_REQUIRE(rowptr && Y, "%s: null rowptr/Y", fn);
  HGD_REQUIRE(X || n_src_rows == 0, "%s: null X", fn);
  *run = true;
  return HGD_OK;
}

template <class TX, class TY>
hgd_status spmm_fill_args(SpmmArgsT<TX, TY>& a, const char* fn, const int64_t* rowptr,
                          const int32_t* col, const float* val, const float* row_scale,
                          int64_t row_begin, int64_t row_end, const TX* X, int64_t ldx, TY* Y,
                          int64_t ldy, int32_t d, int32_t epilogue, float slope,
                          const hgd_row_epilogue* ex, const uint8_t* mask, float keep,
                          const hgd_split_plan* plan, void* workspace, size_t workspace_bytes) {
  const SpmmTuning& t = spmm_tuning();
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
  if (ex) a.ex = *ex;
  a.mask = mask;
  a.keep = keep;
  {
    int e2 = 0;
    a.inv_keep = (!t.mask_div && keep > 0.f && std::frexp(keep, &e2) == 0.5f) ? 1.f / keep : 0.f;
  }
  a.mask_pair = t.mask_pair;
  if (plan && plan->threshold > 0 && plan->n_heavy > 0) {
    HGD_REQUIRE(plan->chunk > 0 && plan->heavy_rows && plan->heavy_cptr && plan->chunk_heavy,
                "%s: incomplete split plan", fn);
    const size_t need = hgd_spmm_workspace_size(plan, d);  // fp32 partials whatever TX / TY
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
  return HGD_OK;
}

// How the columns of a row are cut: a lane owns vec contiguous columns, a group of G lanes one
// row, and a pass (a launch, or one of an interleaved launch's) step = vec·G columns.
struct SpmmPassPlan {
  bool aligned;  // 16-byte rows: the vector path
  int vec, G, step;
};

// sx / sy: element sizes of X and Y; blocked: the source-blocked hop (hgd_spmm_blocked).
inline hgd_status spmm_pass_plan(const char* fn, const void* X, int64_t ldx, size_t sx,
                                 const void* Y, int64_t ldy, size_t sy, int32_t d,
                                 const hgd_row_epilogue* ex, bool blocked, SpmmPassPlan* p) {
  auto al16 = [](const void* ptr, int64_t ld, size_t size) {
    return ptr == nullptr || (reinterpret_cast<uintptr_t>(ptr) % 16 == 0 &&
                              ld % static_cast<int64_t>(16 / size) == 0);
  };
  // fp32: a lane's 4 columns are one 16-byte access. With a 16-bit side a lane owns 8 columns:
  // one access of a bf16 row, two of an fp32 row
  const bool f32 = sx == 4 && sy == 4;
  const int vec = f32 ? 4 : 8;
  bool aligned = al16(X, ldx, sx) && al16(Y, ldy, sy) && d % vec == 0;
  if (ex)
    aligned = aligned && al16(ex->res1, ex->ld_res1, 4) && al16(ex->res2, ex->ld_res2, 4) &&
              al16(ex->act_out, ex->ld_act, 4) && al16(ex->sum_out, ex->ld_sum_out, 4) &&
              al16(ex->sum_res, ex->ld_sum_res, 4);
  if (ex && ex->layer_norm && (aligned ? d > 256 : d > 64))
    return fail(HGD_ERR_UNSUPPORTED,
                "%s: layer_norm needs d <= 256 (16-byte aligned rows) or d <= 64 (got d=%d%s)",
                fn, d, aligned ? "" : ", unaligned");
  p->aligned = aligned;
  if (!aligned) {  // a column per lane
    p->vec = 1;
    p->G = d >= 64 ? 64 : next_pow2(d);
    p->step = p->G;
    return HGD_OK;
  }
  // vector path: one pass when d/vec <= 64 lanes, else 64-lane passes; without a fused epilogue
  // (which needs the whole row in one group) passes are at most pass_cols wide.
  const int lanes = d / vec;
  int G = lanes >= 64 ? 64 : next_pow2(lanes);
  int pass_cols = spmm_tuning().pass_cols;  // HGD_TUNE_SPMM_PASS_COLS overrides every default
  if (pass_cols == 0) {
    if (blocked) {
      // source-blocked: every pass runs the blocks in order, the later ones adding;
      // passes of up to 128 columns: at d = 256 the blocked hop into items takes
      // 16.99 ms in 128-column passes, 18.04 in 64-column ones and 19.54 in one 256-wide pass
      // (scripts/bench_mall_blocked.py --pass-cols, profiles/r06_round/wide/)
      pass_cols = 128;
    } else if (!f32) {
      // 256 B of a bf16 row per gathered piece, the size of the fp32 hop's 64-column piece; with
      // it (or any tuned width, at most 256) a pass of the 8-column path never has 64 lanes
      pass_cols = 128;
    } else {
      // rows up to 128 floats in one pass, wider rows in 64-column passes (measured on MI355X at
      // 100 M edges, d = 256: 64-column passes 64.9 ms per fwd+bwd, 128: 66.3 ms, one 256-wide
      // pass of 64 lanes: 69.4 ms)
      pass_cols = d <= 128 ? 256 : 64;
    }
  }
  if (!ex && vec * G > pass_cols) G = pass_cols / vec;
  p->vec = vec;
  p->G = G;
  p->step = vec * G;
  return HGD_OK;
}

// The column passes of one hop over VEC-column lanes. The fused epilogue (fused), the source
// blocks (blk_seg: the block-major blk_start, n_blk of them over n_rows rows each) and the
// interleaved single launch are fp32-only: HGD_TUNE_SPMM_PASS_INTERLEAVE and
// HGD_TUNE_SPMM_BLOCKED_SEG have no effect on a 16-bit hop.
template <int VEC, class TX, class TY>
hgd_status spmm_passes(SpmmArgsT<TX, TY> a, const SpmmLaunch& L, const SpmmPassPlan& p,
                       bool fused, const int64_t* blk_seg, int32_t n_blk, int64_t n_rows) {
  const int32_t d = a.d, epilogue = a.epi;
  if constexpr (kF32<TX, TY> && VEC == 4) {
    const int n_pass = (d + p.step - 1) / p.step;
    if (spmm_tuning().pass_interleave && n_pass > 1 && !fused && !blk_seg && !a.mask &&
        a.n_chunks == 0 && !a.seg) {
      a.col0 = 0;
      a.n_pass = n_pass;
      a.pass_cols = p.step;
      return launch_vec<VEC, false>(p.G, a, L);
    }
  }
  for (int c0 = 0; c0 < d; c0 += p.step) {
    a.col0 = c0;
    for (int k = 0; k < (blk_seg ? n_blk : 1); ++k) {
      hgd_status s;
      if constexpr (kF32<TX, TY>) {
        if (blk_seg) {
          a.rowptr = blk_seg + static_cast<int64_t>(k) * n_rows;  // block k's own CSR
          if (VEC == 4) a.seg = spmm_tuning().blocked_seg;  // (the vector path's only)
          a.blk_accum = k > 0;
          a.epi = k + 1 == n_blk ? epilogue : HGD_EPI_NONE;  // the activation after the last
        }
        s = fused ? launch_vec<VEC, true>(p.G, a, L) : launch_vec<VEC, false>(p.G, a, L);
      } else {
        s = launch_vec<VEC, false>(p.G, a, L);
      }
      if (s != HGD_OK) return s;
    }
  }
  return HGD_OK;
}

// The hop behind every entry point: fn is the entry point's name, ex the fused row epilogue or
// NULL, mask / keep the edge-dropped view or NULL / 1, and blk_seg (hgd_spmm_blocked) the
// block-major blk_start (rowptr is the same pointer) with col / val the block-major arrays.
template <class TX, class TY>
hgd_status spmm_launch(const int64_t* rowptr, const int32_t* col, const float* val,
                       const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                       int64_t row_begin, int64_t row_end, const TX* X, int64_t ldx, TY* Y,
                       int64_t ldy, int32_t d, int32_t epilogue, float slope,
                       const hgd_row_epilogue* ex, const uint8_t* mask, float keep,
                       const hgd_split_plan* plan, void* workspace, size_t workspace_bytes,
                       void* stream, const char* fn, const int64_t* blk_seg = nullptr,
                       int32_t n_blk = 0, const int32_t* out_row = nullptr) {
  bool run = false;
  hgd_status s = spmm_check_args(fn, rowptr, n_rows, n_src_rows, row_begin, row_end, X, ldx, Y,
                                 ldy, d, epilogue, slope, ex, &run);
  if (s != HGD_OK) return s;
  if (out_row) {
    // the ordered hop (hgd_spmm_ordered) is the row kernel over every row: a split plan's chunks
    // and fix-up and the segmented walk index Y by position, a row range is one of positions, and
    // the fused epilogue's side tables and the blocked hop's passes are indexed by row
    if ((plan && plan->threshold > 0 && plan->n_heavy > 0) ||
        (plan && (plan->flags & HGD_PLAN_SEGMENTED)))
      return fail(HGD_ERR_UNSUPPORTED, "%s: no split rows or segmented walk with a row order", fn);
    if (mask || ex || blk_seg)
      return fail(HGD_ERR_UNSUPPORTED,
                  "%s: no mask, fused row epilogue or source blocks with a row order", fn);
    if (row_begin != 0 || row_end != n_rows)
      return fail(HGD_ERR_UNSUPPORTED, "%s: a row order covers all rows, got [%lld,%lld) of %lld",
                  fn, (long long)row_begin, (long long)row_end, (long long)n_rows);
  }
  if (!run) return s;
  SpmmArgsT<TX, TY> a{};
  s = spmm_fill_args(a, fn, rowptr, col, val, row_scale, row_begin, row_end, X, ldx, Y, ldy, d,
                     epilogue, slope, ex, mask, keep, plan, workspace, workspace_bytes);
  if (s != HGD_OK) return s;
  a.out_row = out_row;
  SpmmPassPlan p;
  s = spmm_pass_plan(fn, X, ldx, sizeof(TX), Y, ldy, sizeof(TY), d, ex, blk_seg != nullptr, &p);
  if (s != HGD_OK) return s;
  const SpmmLaunch L{fn, val != nullptr, as_stream(stream)};
  if (!p.aligned) return spmm_passes<1>(a, L, p, ex != nullptr, blk_seg, n_blk, n_rows);
  return spmm_passes<kF32<TX, TY> ? 4 : 8>(a, L, p, ex != nullptr, blk_seg, n_blk, n_rows);
}

}  // namespace hgd
