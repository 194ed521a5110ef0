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

// The element types the fused row epilogue (EX) is instantiated for: f32→f32 (hgd_spmm_fused) and
// a 16-bit table into an fp32 Y (hgd_spmm_fused_dt).
template <class TX, class TY>
constexpr bool kFusable = std::is_same_v<TY, float>;

// The segmented walk with the fused row epilogue is fp32-only: a fused hop over a 16-bit table
// walks a segmented plan's rows with the row kernel (the same sums, in edge order per row). One
// rule, read at run time where the request is turned into arguments (spmm_fill_args) and at
// compile time where the kernels are instantiated (pick_kernel, launch_g).
template <class TX, class TY>
constexpr bool seg_walk(bool fused) {
  return kF32<TX, TY> || !fused;
}
template <bool EX, class TX, class TY>
constexpr bool kSegWalk = seg_walk<TX, TY>(EX);

// One hop as its extern "C" entry point describes it: the entry point fills a request and calls
// spmm_launch (or spmm_dt.hip's dtype switch), and everything below reads the request. The
// members down to stream are hgd_spmm's arguments in its order, so an entry point initialises
// them from its own in one list; what only some entry points take is named where it is set.
struct SpmmRequest {
  const char* fn;  // the entry point the caller called: the prefix of every error message
  // the structure: CSR of n_rows rows over n_src_rows source rows (val / row_scale: or NULL)
  const int64_t* rowptr;  // NULL for a blocked hop, whose blocks bring their own (blk_start)
  const int32_t* col;
  const float* val;
  const float* row_scale;
  int64_t n_rows, n_src_rows;
  int64_t row_begin, row_end;  // the rows [row_begin, row_end) of Y this call writes
  // the gathered table and the output; spmm_launch's TX / TY say what they point to
  const void* X;
  int64_t ldx;
  void* Y;
  int64_t ldy;
  int32_t d;
  int32_t epilogue;  // HGD_EPI_*
  float slope;
  const hgd_split_plan* plan = nullptr;
  // of the plan's split rows; of a blocked hop into a 16-bit Y, its fp32 partials (blocked_part)
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  void* stream = nullptr;
  const hgd_row_epilogue* ex = nullptr;  // the fused row epilogue
  // ... and, over a 16-bit table (hgd_spmm_fused_dt), the bf16 copy of the rows it writes
  void* y16 = nullptr;
  int64_t ld_y16 = 0;
  // the edge-dropped view (masked: the entry point takes one)
  bool masked = false;
  const uint8_t* mask = nullptr;
  float keep = 1.f;
  // the source blocks (hgd_spmm_blocked): the block-major blk_start, n_blk of them over n_rows
  // rows each, with col / val the block-major arrays
  bool blocked = false;
  const int64_t* blk_start = nullptr;
  int32_t n_blk = 0;
  // the row order (hgd_spmm_ordered and the ordered twins of the fused, masked and 16-bit entry
  // points): position p is written to Y row out_row[p], mask is in the ordered entry order and
  // ex's side tables and y16 stay indexed by Y row. With blocked
  // (hgd_spmm_blocked_ordered) every source block has its own: out_row and row_scale are
  // [n_blk·n_rows], block k's at k·n_rows, in the processing order of its blk_start
  bool ordered = false;
  const int32_t* out_row = nullptr;
  // the blocks' own split plans (hgd_spmm_blocked_split): a host array of n_blk plans, plan k
  // built over block k's CSR (blk_start + k·n_rows), so a row is heavy per block; workspace is
  // then the one chunk-partial buffer the blocks reuse in stream order. plan stays NULL
  const hgd_split_plan* blk_plans = nullptr;
  // packed entries (hgd_spmm_blocked_packed: blocked and ordered): col is the packed word per
  // nonzero, val stays NULL and the weight of code c is dict[c]
  bool packed = false;
  const float* dict = nullptr;
  int32_t n_dict = 0;
  int32_t idx_bits = 0;
};

// Whether n_blocks source blocks over n_src_rows rows (hgd_spmm_col_blocks' cuts: the largest has
// ⌈n_src_rows / n_blocks⌉ rows) and a dictionary of n_dict weights fit one word per nonzero with
// idx_bits bits of block-local column: the one test of the rule, the builder and the hop.
inline bool packed_fits(int64_t n_src_rows, int32_t n_blocks, int64_t n_dict, int32_t idx_bits) {
  if (n_src_rows < 0 || n_blocks < 1 || n_blocks > 64 || idx_bits < 1 || idx_bits > 31) return false;
  const int64_t widest = (n_src_rows + n_blocks - 1) / n_blocks;
  if (widest > (int64_t(1) << idx_bits)) return false;
  const int64_t codes = int64_t(1) << (32 - idx_bits);
  return n_dict >= 1 && n_dict <= codes && n_dict <= HGD_SPMM_PACKED_MAX_DICT;
}

inline hgd_status check_launch(const char* fn, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HGD_ERR_HIP, "%s %s: %s", fn, what, hipGetErrorString(e));
  return HGD_OK;
}

// The kernel of one launch: the masked, the segmented, the ordered or the plain row kernel.
template <bool HAS_VAL, int G, int VEC, int U, int POL, bool EX, class TX, class TY>
auto pick_kernel(const SpmmArgsT<TX, TY>& a, bool seg) {
  if constexpr (POL == kDefaultPolicy && U == 8) {
    // masked (edge-dropped view) hop: the row kernel only, in a row order or not
    if (a.mask) {
      if (a.out_row) return spmm_kernel<G, VEC, U, HAS_VAL, POL, EX, true, TX, TY, true>;
      return spmm_kernel<G, VEC, U, HAS_VAL, POL, EX, true, TX, TY>;
    }
    // the ordered hop with a fused row epilogue and / or a 16-bit side (the plain fp32 one, which
    // carries the tuning matrix, is further down)
    if constexpr (EX || !kF32<TX, TY>) {
      if (a.out_row) return spmm_kernel<G, VEC, U, HAS_VAL, POL, EX, false, TX, TY, true>;
    }
  }
  if constexpr (G >= 8 && kSegWalk<EX, TX, TY>) {
    if (seg) return spmm_seg_kernel<G, VEC, U, HAS_VAL, POL, EX, TX, TY>;
  }
  if constexpr (kF32<TX, TY> && !EX && !HAS_VAL) {
    // the ordered hop over packed entries (its request has no val: the weights are dict's)
    if (a.dict) return spmm_kernel<G, VEC, U, true, POL, false, false, TX, TY, true, true>;
  }
  if constexpr (kF32<TX, TY> && !EX) {
    // the ordered hop (no mask, no segmented walk: spmm_check_args)
    if (a.out_row) return spmm_kernel<G, VEC, U, HAS_VAL, POL, false, false, TX, TY, true>;
  }
  return spmm_kernel<G, VEC, U, HAS_VAL, POL, EX, false, TX, TY>;
}

template <int G, int VEC, int U, int POL, bool EX, class TX, class TY>
void launch_kernel(const SpmmArgsT<TX, TY>& a, const SpmmRequest& r, bool seg, int64_t blocks) {
  auto kernel = r.val ? pick_kernel<true, G, VEC, U, POL, EX>(a, seg)
                      : pick_kernel<false, G, VEC, U, POL, EX>(a, seg);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, as_stream(r.stream), a);
}

template <int G, int VEC, bool EX, class TX, class TY>
void launch_tuned(const SpmmArgsT<TX, TY>& a, const SpmmRequest& r, bool seg, int64_t blocks) {
  if constexpr (kF32<TX, TY> && G == 16 && VEC == 4 && !EX) {
    // the fp32 d = 64 path without a mask carries the tuning matrix (unroll × {plain, nt-store,
    // prefetch, both, prefetch + nt-index, prefetch + nt-index + nt-store})
    if (!a.mask) {
      const SpmmTuning& t = spmm_tuning();
#define HGD_POL_CASES(U)                                                                  \
      switch (t.policy) {                                                                 \
        case 0: return launch_kernel<G, VEC, U, 0, false>(a, r, seg, blocks);             \
        case 1: return launch_kernel<G, VEC, U, 1, false>(a, r, seg, blocks);             \
        case 9: return launch_kernel<G, VEC, U, 9, false>(a, r, seg, blocks);             \
        case 10: return launch_kernel<G, VEC, U, 10, false>(a, r, seg, blocks);           \
        case 11: return launch_kernel<G, VEC, U, 11, false>(a, r, seg, blocks);           \
        default: return launch_kernel<G, VEC, U, 8, false>(a, r, seg, blocks);            \
      }
      if (t.unroll >= 16) { HGD_POL_CASES(16) }
      HGD_POL_CASES(8)
#undef HGD_POL_CASES
    }
  }
  // everything else (a 16-bit side, another width, the fused epilogue, the masked hop): U = 8 with
  // the prefetch policy
  launch_kernel<G, VEC, 8, kDefaultPolicy, EX>(a, r, seg, blocks);
}

// One column pass: the segmented walk, or the row kernel (split-row chunks first in the grid) and
// the fix-up of the split rows.
template <int G, int VEC, bool EX, class TX, class TY>
hgd_status launch_g(SpmmArgsT<TX, TY> a, const SpmmRequest& r) {
  constexpr int GPB = kBlock / G;
  const int64_t rows = a.row_end - a.row_begin;
  if constexpr (G >= 8 && kSegWalk<EX, TX, TY>) {
    if (a.seg) {
      const int64_t sblocks = (rows + static_cast<int64_t>(GPB) * G - 1) / (GPB * G);
      if (sblocks <= 0) return HGD_OK;
      if (sblocks > 0x7fffffffLL) return fail(HGD_ERR_UNSUPPORTED, "%s: grid too large", r.fn);
      launch_tuned<G, VEC, EX>(a, r, true, sblocks);
      return check_launch(r.fn, "segmented kernel");
    }
  }
  int64_t light_blocks = (rows + GPB - 1) / GPB;
  a.heavy_blocks = (a.n_chunks + GPB - 1) / GPB;
  if (a.n_pass > 1) light_blocks = (light_blocks + 7) / 8 * 8 * a.n_pass;  // (no split rows)
  const int64_t blocks = light_blocks + a.heavy_blocks;
  if (blocks > 0) {
    if (blocks > 0x7fffffffLL) return fail(HGD_ERR_UNSUPPORTED, "%s: grid too large", r.fn);
    launch_tuned<G, VEC, EX>(a, r, false, blocks);
    hgd_status s = check_launch(r.fn, "kernel");
    if (s != HGD_OK) return s;
  }
  if (a.n_heavy > 0) {
    if (a.n_heavy > 0x7fffffffLL)
      return fail(HGD_ERR_UNSUPPORTED, "%s: too many split rows", r.fn);
    hipLaunchKernelGGL((spmm_fixup_kernel<G, VEC, EX, TX, TY>), dim3(a.n_heavy), dim3(kBlock), 0,
                       as_stream(r.stream), a);
    return check_launch(r.fn, "fixup");
  }
  return HGD_OK;
}

template <int VEC, bool EX, class TX, class TY>
hgd_status launch_vec(int G, const SpmmArgsT<TX, TY>& a, const SpmmRequest& r) {
  switch (G) {
    case 1: return launch_g<1, VEC, EX>(a, r);
    case 2: return launch_g<2, VEC, EX>(a, r);
    case 4: return launch_g<4, VEC, EX>(a, r);
    case 8: return launch_g<8, VEC, EX>(a, r);
    case 16: return launch_g<16, VEC, EX>(a, r);
    case 32: return launch_g<32, VEC, EX>(a, r);
    case 64:  // a pass of the 8-column path is at most 256 columns: 32 lanes
      if constexpr (VEC != 8) return launch_g<64, VEC, EX>(a, r);
      [[fallthrough]];
    default: return fail(HGD_ERR_UNSUPPORTED, "%s: unsupported group size %d", r.fn, G);
  }
}

// The fp32 scratch a source-blocked hop into a 16-bit Y keeps its running partials in (sy: the
// element size of Y): every row of Y at full width, indexed as Y is, so a row range touches only
// its own rows. 0 for an fp32 Y (it holds its own partial) and for one block.
inline size_t blocked_part_bytes(int64_t n_rows, int32_t d, size_t sy, int32_t n_blk) {
  if (sy != 2 || n_blk <= 1 || n_rows <= 0 || d <= 0) return 0;
  return align_up(static_cast<size_t>(n_rows) * static_cast<size_t>(d) * 4);
}

inline bool has_split_rows(const hgd_split_plan* plan) {
  return plan && plan->threshold > 0 && plan->n_heavy > 0;
}

// Every check that does not depend on the element types, in the order that decides which message
// a call with two faults gets: what a feature of the entry point needs, what every hop needs, and
// what a row order excludes.
inline hgd_status spmm_check_args(const SpmmRequest& r) {
  const char* fn = r.fn;
  const int32_t d = r.d;
  const hgd_row_epilogue* ex = r.ex;
  const bool empty = r.row_end == r.row_begin;
  HGD_REQUIRE(!r.ordered || r.out_row || r.n_rows <= 0, "%s: null %s", fn,
              r.blocked ? "blk_out_row" : "out_row");
  HGD_REQUIRE(!r.blocked || (r.n_blk >= 1 && r.n_blk <= 64), "%s: blocks must be 1..64", fn);
  HGD_REQUIRE(!r.blocked || r.blk_start || r.row_end <= r.row_begin, "%s: null blk_start", fn);
  if (r.packed) {  // (an entry point of its own: blocked and ordered)
    HGD_REQUIRE(r.idx_bits >= 1 && r.idx_bits <= 31, "%s: idx_bits must be 1..31 (got %d)", fn,
                r.idx_bits);
    HGD_REQUIRE(r.n_dict >= 1, "%s: n_dict must be >= 1 (got %d)", fn, r.n_dict);
    HGD_REQUIRE(r.dict || empty, "%s: null dict", fn);
    if (r.n_src_rows >= 0 && !packed_fits(r.n_src_rows, r.n_blk, r.n_dict, r.idx_bits))
      return fail(HGD_ERR_UNSUPPORTED,
                  "%s: %d blocks of %lld source rows and %d weights do not fit %d + %d bits (at "
                  "most %d weights)", fn, r.n_blk, (long long)r.n_src_rows, r.n_dict, r.idx_bits,
                  32 - r.idx_bits, HGD_SPMM_PACKED_MAX_DICT);
  }
  if (r.blocked && r.blk_plans) {
    // a block with split rows is walked by the row kernel, one without by hgd_spmm_blocked's
    // choice (HGD_TUNE_SPMM_BLOCKED_SEG): a plan has no say in it
    for (int32_t k = 0; k < r.n_blk; ++k)
      if (r.blk_plans[k].flags & HGD_PLAN_SEGMENTED)
        return fail(HGD_ERR_UNSUPPORTED, "%s: plan %d is HGD_PLAN_SEGMENTED: no segmented plan "
                    "with source blocks", fn, k);
  }
  HGD_REQUIRE(r.keep > 0.f, "%s: keep must be > 0 (got %g)", fn, (double)r.keep);  // (unmasked: 1)
  HGD_REQUIRE(!r.masked || r.mask || empty, "%s: null mask", fn);
  HGD_REQUIRE(d > 0, "%s: d must be > 0 (got %d)", fn, d);
  HGD_REQUIRE(r.n_rows >= 0 && r.n_src_rows >= 0, "%s: negative sizes", fn);
  HGD_REQUIRE(r.row_begin >= 0 && r.row_begin <= r.row_end && r.row_end <= r.n_rows,
              "%s: row range [%lld,%lld) outside [0,%lld)", fn, (long long)r.row_begin,
              (long long)r.row_end, (long long)r.n_rows);
  HGD_REQUIRE(r.ldx >= d && r.ldy >= d, "%s: ldx/ldy must be >= d", fn);
  HGD_REQUIRE(r.epilogue >= HGD_EPI_NONE && r.epilogue <= HGD_EPI_RELU, "%s: bad epilogue %d", fn,
              r.epilogue);
  if (ex) {
    HGD_REQUIRE(r.epilogue == HGD_EPI_NONE || r.slope >= 0.f,
                "%s: a fused activation needs slope >= 0 (got %g)", fn, (double)r.slope);
    HGD_REQUIRE(ex->layer_norm == 0 || ex->layer_norm == 1, "%s: layer_norm must be 0/1", fn);
    HGD_REQUIRE(!ex->res1 || ex->ld_res1 >= d, "%s: ld_res1 < d", fn);
    HGD_REQUIRE(!ex->res2 || ex->ld_res2 >= d, "%s: ld_res2 < d", fn);
    HGD_REQUIRE(!ex->act_out || ex->ld_act >= d, "%s: ld_act < d", fn);
    HGD_REQUIRE((ex->sum_out == nullptr) == (ex->sum_res == nullptr),
                "%s: sum_out and sum_res go together", fn);
    HGD_REQUIRE(!ex->sum_out || (ex->ld_sum_out >= d && ex->ld_sum_res >= d),
                "%s: ld_sum_out / ld_sum_res < d", fn);
    HGD_REQUIRE(!r.y16 || r.ld_y16 >= d, "%s: ld_y16 < d", fn);
  }
  if (!empty) {
    // col / X may be NULL for a structure without nonzeros (never dereferenced then); a blocked
    // hop's row pointers are its blk_start, checked above
    HGD_REQUIRE((r.rowptr || r.blocked) && r.Y, "%s: null rowptr/Y", fn);
    HGD_REQUIRE(r.X || r.n_src_rows == 0, "%s: null X", fn);
  }
  if (r.out_row) {
    // the ordered hop is the row kernel over every row: a split plan's chunks and fix-up and the
    // segmented walk index Y by position, a row range is one of positions, and the blocked hop's
    // passes are indexed by row — unless the blocks bring their own orders
    // (hgd_spmm_blocked_ordered: blocked and ordered together), which then take neither a mask nor
    // a fused row epilogue. Without blocks both go with an order: the mask is read at the ordered
    // entry position and the epilogue's side tables at the Y row (finish_row)
    if (has_split_rows(r.plan) || (r.plan && (r.plan->flags & HGD_PLAN_SEGMENTED)))
      return fail(HGD_ERR_UNSUPPORTED, "%s: no split rows or segmented walk with a row order", fn);
    if (r.blocked && r.ordered) {
      if (r.mask || ex)
        return fail(HGD_ERR_UNSUPPORTED, "%s: no mask or fused row epilogue with a block order",
                    fn);
    } else if (r.blocked) {
      return fail(HGD_ERR_UNSUPPORTED, "%s: no source blocks with a row order", fn);
    }
    if (r.row_begin != 0 || r.row_end != r.n_rows)
      return fail(HGD_ERR_UNSUPPORTED, "%s: a row order covers all rows, got [%lld,%lld) of %lld",
                  fn, (long long)r.row_begin, (long long)r.row_end, (long long)r.n_rows);
  }
  return HGD_OK;
}

// The kernels' argument block of a request (spmm_passes and launch_g set what changes from launch
// to launch); the split plan is checked here, where its fields are read.
template <class TX, class TY>
hgd_status spmm_fill_args(SpmmArgsT<TX, TY>& a, const SpmmRequest& r) {
  const SpmmTuning& t = spmm_tuning();
  a.rowptr = r.rowptr;
  a.col = r.col;
  a.val = r.val;
  a.row_scale = r.row_scale;
  a.row_begin = r.row_begin;
  a.row_end = r.row_end;
  a.X = static_cast<const TX*>(r.X);
  a.ldx = r.ldx;
  a.Y = static_cast<TY*>(r.Y);
  a.ldy = r.ldy;
  a.d = r.d;
  a.epi = r.epilogue;
  a.slope = r.slope;
  if (r.ex) a.ex = *r.ex;
  a.mask = r.mask;
  a.keep = r.keep;
  int e2 = 0;  // a power of two: the kept weights are multiplied by its exact inverse
  const bool pow2 = !t.mask_div && r.keep > 0.f && std::frexp(r.keep, &e2) == 0.5f;
  a.inv_keep = pow2 ? 1.f / r.keep : 0.f;
  a.mask_pair = t.mask_pair;
  a.out_row = r.out_row;
  if (r.packed) {
    a.dict = r.dict;
    a.n_dict = r.n_dict;
    a.idx_bits = r.idx_bits;
  }
  a.y16 = static_cast<bf16*>(r.y16);
  a.ld_y16 = r.ld_y16;
  const hgd_split_plan* plan = r.plan;
  if (has_split_rows(plan)) {
    HGD_REQUIRE(plan->chunk > 0 && plan->heavy_rows && plan->heavy_cptr && plan->chunk_heavy,
                "%s: incomplete split plan", r.fn);
    const size_t need = hgd_spmm_workspace_size(plan, r.d);  // fp32 partials whatever TX / TY
    if (r.workspace_bytes < need || (need && !r.workspace))
      return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", r.fn, r.workspace_bytes,
                  need);
    a.heavy_threshold = plan->threshold;
    a.chunk = plan->chunk;
    a.n_chunks = plan->n_chunks;
    a.n_heavy = plan->n_heavy;
    a.chunk_heavy = plan->chunk_heavy;
    a.heavy_rows = plan->heavy_rows;
    a.heavy_cptr = plan->heavy_cptr;
    a.partial = static_cast<float*>(r.workspace);
  } else if (plan && (plan->flags & HGD_PLAN_SEGMENTED) && !r.mask &&
             seg_walk<TX, TY>(r.ex != nullptr)) {
    a.seg = 1;  // only without split rows: the segmented walk covers every nonzero of its rows
  }
  if (r.blocked && r.blk_plans) {
    // the blocks' own plans: each checked as the one above; the blocks run in stream order, so
    // the largest one's partials are the workspace (spmm_passes sets a block's plan fields)
    size_t need = 0;
    for (int32_t k = 0; k < r.n_blk; ++k) {
      const hgd_split_plan* bp = r.blk_plans + k;
      if (!has_split_rows(bp)) continue;
      HGD_REQUIRE(bp->chunk > 0 && bp->heavy_rows && bp->heavy_cptr && bp->chunk_heavy,
                  "%s: incomplete split plan of block %d", r.fn, k);
      const size_t nk = hgd_spmm_workspace_size(bp, r.d);
      need = nk > need ? nk : need;
    }
    if (r.workspace_bytes < need || (need && !r.workspace))
      return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", r.fn, r.workspace_bytes,
                  need);
    a.partial = static_cast<float*>(r.workspace);
  }
  if constexpr (sizeof(TY) == 2) {
    if (r.blocked) {  // (a blocked hop has no plan: the workspace is its partials')
      const size_t need = blocked_part_bytes(r.n_rows, r.d, sizeof(TY), r.n_blk);
      if (r.workspace_bytes < need || (need && !r.workspace))
        return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", r.fn, r.workspace_bytes,
                    need);
      a.blk_part = need ? static_cast<float*>(r.workspace) : nullptr;
      a.ld_part = r.d;
    }
  }
  return HGD_OK;
}

// How the columns of a row are cut: a lane owns vec contiguous columns, a group of G lanes one
// row, and a pass (a launch, or one of an interleaved launch's) step = vec·G columns.
struct SpmmPassPlan {
  bool aligned;  // 16-byte rows: the vector path
  int G, step;
};

// sx / sy: element sizes of X and Y.
inline hgd_status spmm_pass_plan(const SpmmRequest& r, size_t sx, size_t sy, SpmmPassPlan* p) {
  const int32_t d = r.d;
  const hgd_row_epilogue* ex = r.ex;
  auto al16 = [](const void* ptr, int64_t ld, size_t size) {
    return ptr == nullptr || (reinterpret_cast<uintptr_t>(ptr) % 16 == 0 &&
                              ld % static_cast<int64_t>(16 / size) == 0);
  };
  // fp32: a lane's 4 columns are one 16-byte access. With a 16-bit side a lane owns 8 columns:
  // one access of a bf16 row, two of an fp32 row
  const bool f32 = sx == 4 && sy == 4;
  const int vec = f32 ? 4 : 8;
  bool aligned = al16(r.X, r.ldx, sx) && al16(r.Y, r.ldy, sy) && d % vec == 0;
  // (the partials of a blocked hop into a 16-bit Y: fp32 rows of d)
  if (r.blocked && sy == 2 && r.n_blk > 1) aligned = aligned && al16(r.workspace, d, 4);
  if (ex)
    aligned = aligned && al16(ex->res1, ex->ld_res1, 4) && al16(ex->res2, ex->ld_res2, 4) &&
              al16(ex->act_out, ex->ld_act, 4) && al16(ex->sum_out, ex->ld_sum_out, 4) &&
              al16(ex->sum_res, ex->ld_sum_res, 4) && al16(r.y16, r.ld_y16, 2);
  if (ex && ex->layer_norm && (aligned ? d > 256 : d > 64))
    return fail(HGD_ERR_UNSUPPORTED,
                "%s: layer_norm needs d <= 256 (16-byte aligned rows) or d <= 64 (got d=%d%s)",
                r.fn, d, aligned ? "" : ", unaligned");
  p->aligned = aligned;
  if (!aligned) {  // a column per lane
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
    if (r.blocked && r.blk_plans && r.n_blk == 1) {
      // one block with its plan is hgd_spmm with that plan, bit for bit: the fix-up's combine
      // order is fixed by the lanes per row, so it takes hgd_spmm's passes (below)
      pass_cols = d <= 128 ? 256 : 64;
    } else if (r.blocked) {
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
  // (a fused row wider than 256 columns, which has no LayerNorm: 256-column passes of 32 lanes)
  if (ex && !f32 && G > 32) G = 32;
  p->G = G;
  p->step = vec * G;
  return HGD_OK;
}

// The column passes of one hop over VEC-column lanes. The fused epilogue needs an fp32 Y (over a
// 16-bit table: hgd_spmm_fused_dt) and the interleaved single launch is fp32-only, as is the
// segmented walk of a source block's rows:
// HGD_TUNE_SPMM_PASS_INTERLEAVE and HGD_TUNE_SPMM_BLOCKED_SEG have no effect on a 16-bit hop.
template <int VEC, class TX, class TY>
hgd_status spmm_passes(SpmmArgsT<TX, TY> a, const SpmmRequest& r, const SpmmPassPlan& p) {
  const int32_t d = a.d;
  const bool fused = r.ex != nullptr;
  if constexpr (kF32<TX, TY> && VEC == 4) {
    const int n_pass = (d + p.step - 1) / p.step;
    if (spmm_tuning().pass_interleave && n_pass > 1 && !fused && !r.blocked && !a.mask &&
        a.n_chunks == 0 && !a.seg) {
      a.col0 = 0;
      a.n_pass = n_pass;
      a.pass_cols = p.step;
      return launch_vec<VEC, false>(p.G, a, r);
    }
  }
  for (int c0 = 0; c0 < d; c0 += p.step) {
    a.col0 = c0;
    for (int k = 0; k < (r.blocked ? r.n_blk : 1); ++k) {
      hgd_status s;
      if (r.blocked) {
        a.rowptr = r.blk_start + static_cast<int64_t>(k) * r.n_rows;  // block k's own CSR
        if (r.ordered) {  // ... in its own row order (the row kernel only: no segmented walk)
          a.out_row = r.out_row + static_cast<int64_t>(k) * r.n_rows;
          if (r.row_scale) a.row_scale = r.row_scale + static_cast<int64_t>(k) * r.n_rows;
          if (r.packed)  // a packed column counts from the block's first source row
            a.X = static_cast<const TX*>(r.X) + r.n_src_rows * k / r.n_blk * r.ldx;
        } else if constexpr (kF32<TX, TY>) {
          if (VEC == 4) a.seg = spmm_tuning().blocked_seg;  // (the vector path's only)
        }
        if (r.blk_plans) {
          // block k's own split plan: its chunks lead this launch's grid and its fix-up follows
          // (launch_g), both over the one workspace; a piece of a row is written once per block,
          // by the row kernel when it is light in this block and by the fix-up when it is heavy
          const hgd_split_plan* bp = r.blk_plans + k;
          const bool split = has_split_rows(bp);
          a.heavy_threshold = split ? bp->threshold : 0;
          a.chunk = split ? bp->chunk : 0;
          a.n_chunks = split ? bp->n_chunks : 0;
          a.n_heavy = split ? bp->n_heavy : 0;
          a.chunk_heavy = split ? bp->chunk_heavy : nullptr;
          a.heavy_rows = split ? bp->heavy_rows : nullptr;
          a.heavy_cptr = split ? bp->heavy_cptr : nullptr;
          if (split) a.seg = 0;  // the segmented walk covers every nonzero of its rows
        }
        a.blk_accum = k > 0;
        a.epi = k + 1 == r.n_blk ? r.epilogue : HGD_EPI_NONE;  // the activation after the last
        a.blk_last = k + 1 == r.n_blk;  // (read for a 16-bit Y only: it then leaves the scratch)
      }
      if constexpr (kFusable<TX, TY>) {
        s = fused ? launch_vec<VEC, true>(p.G, a, r) : launch_vec<VEC, false>(p.G, a, r);
      } else {
        s = launch_vec<VEC, false>(p.G, a, r);
      }
      if (s != HGD_OK) return s;
    }
  }
  return HGD_OK;
}

// The hop behind every entry point, over a table of TX and an output of TY.
template <class TX, class TY>
hgd_status spmm_launch(const SpmmRequest& r) {
  hgd_status s = spmm_check_args(r);
  if (s != HGD_OK || r.row_end == r.row_begin) return s;  // (an empty range: nothing to launch)
  SpmmArgsT<TX, TY> a{};
  s = spmm_fill_args(a, r);
  if (s != HGD_OK) return s;
  SpmmPassPlan p;
  s = spmm_pass_plan(r, sizeof(TX), sizeof(TY), &p);
  if (s != HGD_OK) return s;
  if (!p.aligned) return spmm_passes<1>(a, r, p);
  return spmm_passes<kF32<TX, TY> ? 4 : 8>(a, r, p);
}

}  // namespace hgd
