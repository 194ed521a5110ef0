// KHGRec's view-fusion attention on the device (include/hgd.h, "View attention"):
//   hgd_view_attention_forward   Attention.forward (KHGRec.py:466-480; call sites :132, :202)
//   hgd_view_attention_backward  its gradients: the two views' rows, and W1 / b1 / W2 on request
// The reference stacks the views ([N, 2, d]), runs Linear → Tanh → Linear on both, a softmax
// over the two views and the weighted sum: five [N, 2, d] intermediates. Here a workgroup owns
// kVaRows rows, stages both views once, and keeps t_v, t_0 − t_1, q and β on chip. The three
// products (forward) and five (backward) run on the bf16 MFMA with every f32 operand cut exactly
// into three bf16 terms (linear_common.h): error ≈ 1e-7·Σ|a·b|. Every sum has a fixed order and
// a row's results depend on nothing but the row: two runs are bitwise equal, at any N.
//
// Weights: each wave owns one 16-column tile of every product and holds that tile's split
// fragments of W1 and W2 (the backward: W1, W2ᵀ-side and W1ᵀ-side) in REGISTERS for the whole
// launch — 48 VGPRs per matrix at d = 128 — read once per workgroup through the cache. LDS holds
// only rows: the views as f32 (the epilogue's operands) and as bf16 planes in MFMA-fragment
// order, and one more operand's planes (t_0 − t_1, or dq).
#include "view_attention_tile.h"

namespace hgd {
namespace {

struct VaFwd {
  const float* z[2];
  int64_t ld[2];
  int64_t n;
  int32_t d;
  const float *W1, *b1, *W2;
  float* out;
  int64_t ldo;
  float* beta0;  // NULL: not stored (eval)
  int64_t ldb;
};

// ---- forward --------------------------------------------------------------------------------
// Wave (ct, rt0): column tile ct of row tiles rt0, rt0 + RTW; lane (i16, g): row i16 of the tile,
// columns 16·ct + 4g .. + 3.
template <int KQ>
__global__ __launch_bounds__(VA<KQ>::THREADS) void k_va_forward(VaFwd p) {
  using C = VA<KQ>;
  extern __shared__ __align__(16) char va_smem[];
  char* Zp = va_smem + 2 * C::F32_BYTES;  // [2 views][3][plane]
  char* Dp = Zp + 2 * C::OPER_BYTES;      // t_0 − t_1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int ct = wave % C::NCT, rt0 = wave / C::NCT;
  const int col0 = 16 * ct + 4 * g;
  const bool live = 16 * ct < p.d;

  bf16x8 w1[KQ][3], w2[KQ][3];
  load_wfrag<KQ>(p.W1, p.d, 1, p.d, 16 * ct + i16, g, w1);  // Bm[k][n] = W1[n][k]
  load_wfrag<KQ>(p.W2, p.d, 1, p.d, 16 * ct + i16, g, w2);
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (live) bias = f32x4{p.b1[col0], p.b1[col0 + 1], p.b1[col0 + 2], p.b1[col0 + 3]};

  const float* const src[2] = {p.z[0], p.z[1]};
  const int64_t lds[2] = {p.ld[0], p.ld[1]};
  const int64_t nblocks = (p.n + kVaRows - 1) / kVaRows;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t r0 = blk * kVaRows;
    __syncthreads();  // the previous block's rows and planes are read
    {
      f32x4 v[Stage<KQ, 2>::F];
      load_block<KQ, 2>(src, lds, r0, p.n, p.d, v);
      store_block<KQ, 2>(v, va_smem, Zp);
    }
    __syncthreads();
#pragma unroll
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const f32x4 t0 = tanh4(tile_product<KQ>(Zp, rt, i16, g, w1) + bias);
      const f32x4 t1 = tanh4(tile_product<KQ>(Zp + C::OPER_BYTES, rt, i16, g, w1) + bias);
      put_planes<KQ>(Dp, 16 * rt + i16, 4 * ct + g, t0 - t1);  // a dead tile: exact zeros
    }
    __syncthreads();
#pragma unroll
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const f32x4 q = tile_product<KQ>(Dp, rt, i16, g, w2);
      const int rl = 16 * rt + i16;
      const f32x4 z0 = *reinterpret_cast<const f32x4*>(va_smem + (rl * C::LDF + col0) * 4);
      const f32x4 z1 =
          *reinterpret_cast<const f32x4*>(va_smem + C::F32_BYTES + (rl * C::LDF + col0) * 4);
      f32x4 b0, o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        b0[j] = sigmoid_stable(q[j]);
        o[j] = fmaf(b0[j], z0[j], (1.f - b0[j]) * z1[j]);
      }
      const int64_t row = r0 + rl;
      if (live && row < p.n) {
        *reinterpret_cast<f32x4*>(p.out + row * p.ldo + col0) = o;
        if (p.beta0) *reinterpret_cast<f32x4*>(p.beta0 + row * p.ldb + col0) = b0;
      }
    }
  }
}

struct VaBwd {
  const float* z[2];
  int64_t ld[2];
  const float* g;
  int64_t ldg;
  const float* beta0;
  int64_t ldb;
  int64_t n;
  int32_t d;
  const float *W1, *b1, *W2;
  float* dz[2];  // both or neither
  int64_t lddz[2];
  float* ops;    // NULL, or [4][n, d]: dq, t_0 − t_1, da_0, da_1 for the parameter products
  int64_t op_stride;  // floats between two of them
};

// ---- backward-data --------------------------------------------------------------------------
// Phase A: t_v again (two products), dq → planes. Phase B: h = dq·W2, da_v → the views' planes
// (their last reads were phase A's). Phase C: dz_v = β_v ⊙ g + da_v·W1.
template <int KQ>
__global__ __launch_bounds__(VA<KQ>::THREADS) void k_va_backward(VaBwd p) {
  using C = VA<KQ>;
  extern __shared__ __align__(16) char va_smem[];
  char* Zp = va_smem + 4 * C::F32_BYTES;  // [2][3][plane]: the views, then da_0 / da_1
  char* Dp = Zp + 2 * C::OPER_BYTES;      // dq
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int ct = wave % C::NCT, rt0 = wave / C::NCT;
  const int col0 = 16 * ct + 4 * g;
  const bool live = 16 * ct < p.d;
  const bool want_rows = p.dz[0] != nullptr;

  bf16x8 w1[KQ][3], w2t[KQ][3], w1t[KQ][3];
  load_wfrag<KQ>(p.W1, p.d, 1, p.d, 16 * ct + i16, g, w1);   // Bm[k][n] = W1[n][k]
  load_wfrag<KQ>(p.W2, p.d, p.d, 1, 16 * ct + i16, g, w2t);  // Bm[k][n] = W2[k][n]
  load_wfrag<KQ>(p.W1, p.d, p.d, 1, 16 * ct + i16, g, w1t);  // Bm[k][n] = W1[k][n]
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (live) bias = f32x4{p.b1[col0], p.b1[col0 + 1], p.b1[col0 + 2], p.b1[col0 + 3]};

  const float* const src[4] = {p.z[0], p.z[1], p.g, p.beta0};
  const int64_t lds[4] = {p.ld[0], p.ld[1], p.ldg, p.ldb};
  const int64_t nblocks = (p.n + kVaRows - 1) / kVaRows;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t r0 = blk * kVaRows;
    __syncthreads();  // the previous block's rows and planes are read
    {
      f32x4 v[Stage<KQ, 4>::F];
      load_block<KQ, 4>(src, lds, r0, p.n, p.d, v);
      store_block<KQ, 4>(v, va_smem, Zp);
    }
    __syncthreads();
    // (the row-tile loops stay rolled: unrolled, the second tile's fragments and 1 − t_v² on top
    // of the 144 registers of weights did not fit 256)
#pragma unroll 1
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const int rl = 16 * rt + i16;
      const f32x4 t0 = tanh4(tile_product<KQ>(Zp, rt, i16, g, w1) + bias);
      const f32x4 t1 = tanh4(tile_product<KQ>(Zp + C::OPER_BYTES, rt, i16, g, w1) + bias);
      const int at = (rl * C::LDF + col0) * 4;
      f32x4* z0p = reinterpret_cast<f32x4*>(va_smem + at);
      f32x4* z1p = reinterpret_cast<f32x4*>(va_smem + C::F32_BYTES + at);
      const f32x4 gg = *reinterpret_cast<const f32x4*>(va_smem + 2 * C::F32_BYTES + at);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(va_smem + 3 * C::F32_BYTES + at);
      const f32x4 dq = gg * (*z0p - *z1p) * (b0 * (1.f - b0));
      // 1 − t_v² waits for phase B where this lane read z_v (no other lane touches the piece)
      *z0p = 1.f - t0 * t0;
      *z1p = 1.f - t1 * t1;
      put_planes<KQ>(Dp, rl, 4 * ct + g, dq);
      const int64_t row = r0 + rl;
      if (p.ops && live && row < p.n) {
        float* o = p.ops + row * p.d + col0;
        *reinterpret_cast<f32x4*>(o) = dq;
        *reinterpret_cast<f32x4*>(o + p.op_stride) = t0 - t1;
      }
    }
    __syncthreads();  // dq is whole; the views' planes are read
#pragma unroll 1
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const int rl = 16 * rt + i16;
      const f32x4 h = tile_product<KQ>(Dp, rt, i16, g, w2t);
      const int at = (rl * C::LDF + col0) * 4;
      const f32x4 da0 = h * *reinterpret_cast<const f32x4*>(va_smem + at);
      const f32x4 da1 = -(h * *reinterpret_cast<const f32x4*>(va_smem + C::F32_BYTES + at));
      put_planes<KQ>(Zp, rl, 4 * ct + g, da0);
      put_planes<KQ>(Zp + C::OPER_BYTES, rl, 4 * ct + g, da1);
      const int64_t row = r0 + rl;
      if (p.ops && live && row < p.n) {
        float* o = p.ops + 2 * p.op_stride + row * p.d + col0;
        *reinterpret_cast<f32x4*>(o) = da0;
        *reinterpret_cast<f32x4*>(o + p.op_stride) = da1;
      }
    }
    if (!want_rows) continue;  // (uniform)
    __syncthreads();  // da_0, da_1 are whole
#pragma unroll 1
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const int rl = 16 * rt + i16;
      const f32x4 p0 = tile_product<KQ>(Zp, rt, i16, g, w1t);
      const f32x4 p1 = tile_product<KQ>(Zp + C::OPER_BYTES, rt, i16, g, w1t);
      const int at = (rl * C::LDF + col0) * 4;
      const f32x4 gg = *reinterpret_cast<const f32x4*>(va_smem + 2 * C::F32_BYTES + at);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(va_smem + 3 * C::F32_BYTES + at);
      f32x4 d0, d1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d0[j] = fmaf(b0[j], gg[j], p0[j]);
        d1[j] = fmaf(1.f - b0[j], gg[j], p1[j]);
      }
      const int64_t row = r0 + rl;
      if (live && row < p.n) {
        *reinterpret_cast<f32x4*>(p.dz[0] + row * p.lddz[0] + col0) = d0;
        *reinterpret_cast<f32x4*>(p.dz[1] + row * p.lddz[1] + col0) = d1;
      }
    }
  }
}

template <int KQ>
hgd_status launch_forward(const VaFwd& p, hipStream_t st, const char* fn) {
  using C = VA<KQ>;
  static int resident[kMaxDevices] = {};
  int cap = 0;
  if (hgd_status s = resident_blocks(k_va_forward<KQ>, C::THREADS, C::LDS_FWD, resident, &cap))
    return s;
  const int64_t nblocks = (p.n + kVaRows - 1) / kVaRows;
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>(nblocks, cap));
  hipLaunchKernelGGL(k_va_forward<KQ>, dim3(grid), dim3(C::THREADS), C::LDS_FWD, st, p);
  return check_launch(fn);
}

template <int KQ>
hgd_status launch_backward(const VaBwd& p, hipStream_t st, const char* fn) {
  using C = VA<KQ>;
  static int resident[kMaxDevices] = {};
  int cap = 0;
  if (hgd_status s = resident_blocks(k_va_backward<KQ>, C::THREADS, C::LDS_BWD, resident, &cap))
    return s;
  const int64_t nblocks = (p.n + kVaRows - 1) / kVaRows;
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>(nblocks, cap));
  hipLaunchKernelGGL(k_va_backward<KQ>, dim3(grid), dim3(C::THREADS), C::LDS_BWD, st, p);
  return check_launch(fn);
}

hgd_status check_common(const char* fn, const float* z0, int64_t ld0, const float* z1,
                        int64_t ld1, int64_t n, int32_t d, const float* W1, const float* b1,
                        const float* W2) {
  HGD_REQUIRE(d >= 16 && d <= 128 && d % 16 == 0,
              "%s: d = %d is not a fused width (a multiple of 16 in [16, 128])", fn, d);
  HGD_REQUIRE(n >= 0 && n < (int64_t{1} << 40), "%s: n_rows out of range", fn);
  HGD_REQUIRE(ld0 >= d && ld1 >= d, "%s: the views' leading dimensions must be >= d", fn);
  HGD_REQUIRE(z0 && z1 && W1 && b1 && W2, "%s: null pointer", fn);
  HGD_REQUIRE(al16r(z0, ld0) && al16r(z1, ld1), "%s: the views' rows must be 16-byte aligned", fn);
  return HGD_OK;
}

// The parameter path's workspace: the four operands, the second view's dW1 / db1 terms, and
// hgd_gemm_tn's split-K partials (the larger of the two calls).
struct ParamPlan {
  size_t op_bytes, tmp_bytes, tn_bytes;
  hgd_gemm_tn_desc w1[2], w2;
};

ParamPlan param_plan(int64_t n, int32_t d, const float* z0, int64_t ld0, const float* z1,
                     int64_t ld1, char* ws, float* dW1, float* db1, float* dW2) {
  ParamPlan pl{};
  pl.op_bytes = align_up(static_cast<size_t>(n) * d * sizeof(float));
  pl.tmp_bytes = align_up((static_cast<size_t>(d) * d + d) * sizeof(float));
  float* ops = reinterpret_cast<float*>(ws);
  const size_t stride = pl.op_bytes / sizeof(float);
  float* tmp = reinterpret_cast<float*>(ws + 4 * pl.op_bytes);
  for (int v = 0; v < 2; ++v) {
    hgd_gemm_tn_desc& e = pl.w1[v];
    e.A = ops + (2 + v) * stride;  // da_v
    e.lda = d;
    e.B = v == 0 ? z0 : z1;
    e.ldb = v == 0 ? ld0 : ld1;
    e.rows = n;
    e.M = e.N = d;
    e.C = v == 0 ? dW1 : tmp;
    e.colsum_A = v == 0 ? db1 : tmp + static_cast<size_t>(d) * d;
  }
  pl.w2.A = ops;  // dq
  pl.w2.lda = d;
  pl.w2.B = ops + stride;  // t_0 − t_1
  pl.w2.ldb = d;
  pl.w2.rows = n;
  pl.w2.M = pl.w2.N = d;
  pl.w2.C = dW2;
  pl.tn_bytes = std::max(hgd_gemm_tn_workspace_size(pl.w1, 2),
                         hgd_gemm_tn_workspace_size(&pl.w2, 1));
  return pl;
}

}  // namespace
}  // namespace hgd

using namespace hgd;

extern "C" int32_t hgd_view_attention_row_block(void) { return kVaRows; }

extern "C" size_t hgd_view_attention_workspace_size(int64_t n_rows, int32_t d, int64_t ld0,
                                                    int64_t ld1) {
  if (n_rows <= 0 || d < 16 || d > 128 || d % 16 != 0 || ld0 < d || ld1 < d) return 0;
  // placeholders with the alignment the calls require: only sizes are read
  float* const a16 = reinterpret_cast<float*>(uintptr_t{256});
  const ParamPlan pl =
      param_plan(n_rows, d, a16, ld0, a16, ld1, reinterpret_cast<char*>(a16), a16, a16, a16);
  return 4 * pl.op_bytes + pl.tmp_bytes + pl.tn_bytes;
}

extern "C" hgd_status hgd_view_attention_forward(const float* z0, int64_t ld0, const float* z1,
                                                 int64_t ld1, int64_t n_rows, int32_t d,
                                                 const float* W1, const float* b1,
                                                 const float* W2, float* out, int64_t ldo,
                                                 float* beta0, int64_t ldb, void* stream) {
  clear_error();
  const char* fn = "hgd_view_attention_forward";
  if (hgd_status st = check_common(fn, z0, ld0, z1, ld1, n_rows, d, W1, b1, W2)) return st;
  HGD_REQUIRE(out, "%s: null pointer", fn);
  HGD_REQUIRE(ldo >= d && (!beta0 || ldb >= d), "%s: ldo / ldb must be >= d", fn);
  HGD_REQUIRE(al16r(out, ldo) && (!beta0 || al16r(beta0, ldb)),
              "%s: the rows of out / beta0 must be 16-byte aligned", fn);
  if (n_rows == 0) return HGD_OK;
  const VaFwd p{{z0, z1}, {ld0, ld1}, n_rows, d, W1, b1, W2, out, ldo, beta0, ldb};
  hipStream_t st = as_stream(stream);
  switch ((d + 31) / 32) {
    case 1: return launch_forward<1>(p, st, fn);
    case 2: return launch_forward<2>(p, st, fn);
    case 3: return launch_forward<3>(p, st, fn);
    default: return launch_forward<4>(p, st, fn);
  }
}

extern "C" hgd_status hgd_view_attention_backward(
    const float* z0, int64_t ld0, const float* z1, int64_t ld1, int64_t n_rows, int32_t d,
    const float* W1, const float* b1, const float* W2, const float* beta0, int64_t ldb,
    const float* g, int64_t ldg, float* dz0, int64_t lddz0, float* dz1, int64_t lddz1,
    float* dW1, float* db1, float* dW2, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  const char* fn = "hgd_view_attention_backward";
  if (hgd_status st = check_common(fn, z0, ld0, z1, ld1, n_rows, d, W1, b1, W2)) return st;
  HGD_REQUIRE(beta0 && g, "%s: null pointer", fn);
  HGD_REQUIRE(ldb >= d && ldg >= d, "%s: ldb / ldg must be >= d", fn);
  HGD_REQUIRE(al16r(beta0, ldb) && al16r(g, ldg),
              "%s: the rows of beta0 / g must be 16-byte aligned", fn);
  HGD_REQUIRE((dz0 == nullptr) == (dz1 == nullptr), "%s: dz0 and dz1 go together", fn);
  HGD_REQUIRE(!dz0 || (lddz0 >= d && lddz1 >= d), "%s: lddz0 / lddz1 must be >= d", fn);
  HGD_REQUIRE(!dz0 || (al16r(dz0, lddz0) && al16r(dz1, lddz1)),
              "%s: the rows of dz0 / dz1 must be 16-byte aligned", fn);
  const bool params = dW1 != nullptr;
  HGD_REQUIRE(params == (db1 != nullptr) && params == (dW2 != nullptr),
              "%s: dW1, db1 and dW2 go together", fn);
  HGD_REQUIRE(dz0 || params, "%s: nothing to compute (no dz, no parameter gradients)", fn);
  ParamPlan pl{};
  if (params && n_rows > 0) {
    HGD_REQUIRE(workspace && al16p(workspace), "%s: null or misaligned workspace", fn);
    pl = param_plan(n_rows, d, z0, ld0, z1, ld1, static_cast<char*>(workspace), dW1, db1, dW2);
    const size_t need = 4 * pl.op_bytes + pl.tmp_bytes + pl.tn_bytes;
    HGD_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < required %zu", fn, workspace_bytes,
                need);
  }
  if (n_rows == 0) return HGD_OK;
  VaBwd p{{z0, z1}, {ld0, ld1}, g, ldg, beta0, ldb, n_rows, d, W1, b1, W2,
          {dz0, dz1}, {lddz0, lddz1}, nullptr, 0};
  if (params) {
    p.ops = static_cast<float*>(workspace);
    p.op_stride = static_cast<int64_t>(pl.op_bytes / sizeof(float));
  }
  hipStream_t st = as_stream(stream);
  hgd_status ls;
  switch ((d + 31) / 32) {
    case 1: ls = launch_backward<1>(p, st, fn); break;
    case 2: ls = launch_backward<2>(p, st, fn); break;
    case 3: ls = launch_backward<3>(p, st, fn); break;
    default: ls = launch_backward<4>(p, st, fn); break;
  }
  if (ls != HGD_OK || !params) return ls;
  // dW1 = da_0ᵀ·z0 + da_1ᵀ·z1, db1 = Σ_rows (da_0 + da_1), dW2 = dqᵀ·(t_0 − t_1): split-K with
  // the slices summed in slice order (hgd_gemm_tn)
  char* tn_ws = static_cast<char*>(workspace) + 4 * pl.op_bytes + pl.tmp_bytes;
  if (hgd_status s = hgd_gemm_tn(pl.w1, 2, tn_ws, pl.tn_bytes, stream)) return s;
  const int nW = d * d;
  hipLaunchKernelGGL(k_va_add, dim3(grid_for(nW + d)), dim3(kBlock), 0, st, dW1, pl.w1[1].C, nW,
                     db1, pl.w1[1].colsum_A, d);
  if (hgd_status s = check_launch(fn)) return s;
  return hgd_gemm_tn(&pl.w2, 1, tn_ws, pl.tn_bytes, stream);
}
