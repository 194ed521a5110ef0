// KHGRec's CF loss on the device over the batch's item rows only (include/hgd.h, "CF loss"):
//   hgd_cf_loss_forward   the view fusion at the 2B positions named by pid / nid, the BPR loss
//                         and the regulariser (KHGRec.py:131-143, :341-345)
//   hgd_cf_loss_backward  its gradients per position: DA [B, d], DZ0 / DZ1 [2B, d], and
//                         W1 / b1 / W2 on request
// The reference fuses EVERY item row and gathers 2B of them. Here a workgroup owns 32 positions
// (16 triples; position 2k is triple k's positive, 2k + 1 its negative), reads both views through
// the ids, runs the view attention's tile code on them (view_attention_tile.h) and keeps the fused
// rows F and their gradient dF in LDS: nothing of size n_items·d is touched. Every sum has a
// fixed order, no float atomics: two runs are bitwise equal, and a triple's coef and gradients
// depend on that triple's rows and the three norms alone.
//
// Registers: the backward forms dF as a phase of its own (a float4 piece of one triple per
// thread) that writes the LDS rows k_va_backward stages dOut into; from there on it is
// k_va_backward's three phases, so the 144 registers of weight fragments meet no new live values.
#include <cmath>

#include "view_attention_tile.h"

namespace hgd {
namespace {

constexpr int kCfTriples = kVaRows / 2;  // triples of a workgroup's block
constexpr int kCfPart = 4;               // a block's partial sums: Σℓ, Σa², Σp², Σn²
constexpr float kBprEps = 1e-5f;         // bpr_loss's 10e-6 (util/loss_torch.py:8)

struct CfIn {
  const float* U;
  int64_t ldu;
  const int32_t* uid;
  const float* z[2];
  int64_t ld[2];
  const int32_t *pid, *nid;
  int64_t B;
  int32_t d;
  const float *W1, *b1, *W2;  // all NULL: the mean of the two views
};

struct CfFwd {
  CfIn in;
  float* beta0;  // [2B, d] or NULL (no backward to follow, or mean mode)
  int64_t ldb;
  float* coef;   // [B]
  float* part;   // [blocks][kCfPart]
};

struct CfBwd {
  CfIn in;
  const float* beta0;
  int64_t ldb;
  const float *coef, *norms, *grad;
  float lam;  // reg / batch_size
  float* dA;  // NULL: not computed
  int64_t ldda;
  float* dz[2];  // both or neither
  int64_t lddz[2];
  float* ops;  // NULL, or [6][2B, d]: dq, t_0 − t_1, da_0, da_1, and the staged rows of z0, z1
  int64_t op_stride;
};

// ℓ = −log(ε + σ(x)) and c = −dℓ/dx = σ(x)σ(−x)/(ε + σ(x)), both sigmoids from one exponential
// of −|x| <= 0 (finite, and σ(−x) keeps its digits when σ(x) rounds to 1)
__device__ __forceinline__ void bpr_terms(float x, float& l, float& c) {
  const float e = expf(-fabsf(x));
  const float s = (x >= 0.f ? 1.f : e) / (1.f + e);
  const float sm = (x >= 0.f ? e : 1.f) / (1.f + e);
  l = -logf(kBprEps + s);
  c = s * sm / (kBprEps + s);
}

// The per-gradient scalars: g/B, and g·λ/‖·‖ of (A, P, N), 0 where the norm is 0 (torch.norm's
// backward at 0)
struct CfScale {
  float gB, sA, sP, sN;
};

__device__ __forceinline__ CfScale load_scale(const CfBwd& p) {
  const float g = p.grad[0];
  CfScale s;
  s.gB = g / static_cast<float>(p.in.B);
  s.sA = p.norms[0] > 0.f ? g * p.lam / p.norms[0] : 0.f;
  s.sP = p.norms[1] > 0.f ? g * p.lam / p.norms[1] : 0.f;
  s.sN = p.norms[2] > 0.f ? g * p.lam / p.norms[2] : 0.f;
  return s;
}

// The block's row numbers: the item of each of its 32 positions and the user of each of its 16
// triples (slots past the batch's end: row 0, whose values are never used)
__device__ __forceinline__ void block_ids(const CfIn& in, int64_t t0, int n_tr, int* sh_item,
                                          int* sh_user) {
  const int t = threadIdx.x;
  if (t < kVaRows) {
    const int k = t >> 1;
    sh_item[t] = k < n_tr ? ((t & 1) ? in.nid[t0 + k] : in.pid[t0 + k]) : 0;
  } else if (t < kVaRows + kCfTriples) {
    const int k = t - kVaRows;
    sh_user[k] = k < n_tr ? in.uid[t0 + k] : 0;
  }
}

// load_block through the ids: this thread's float4 pieces of the two views' rows sh_item[·]
// (zeros past position n_pos and column d: a clamped load and a select)
template <int KQ>
__device__ __forceinline__ void load_views(const CfIn& in, const int* sh_item, int n_pos,
                                           f32x4 (&v)[Stage<KQ, 2>::F]) {
  using S = Stage<KQ, 2>;
#pragma unroll
  for (int u = 0; u < S::F; ++u) {
    const int f = threadIdx.x + S::C::THREADS * u;
    const int a = f / S::PER, rem = f % S::PER;
    const int rl = rem / S::C::LPR, c = rem % S::C::LPR;
    const bool ok = rl < n_pos && 4 * c < in.d;
    v[u] = ld4(in.z[a] + (ok ? static_cast<int64_t>(sh_item[rl]) * in.ld[a] + 4 * c : 0));
    if (!ok) v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// The block's 16 anchor rows U[sh_user[·]] → f32 rows in LDS (stride LDF)
template <int KQ>
__device__ __forceinline__ void stage_anchors(const CfIn& in, const int* sh_user, int n_tr,
                                              char* An) {
  using C = VA<KQ>;
#pragma unroll 1
  for (int f = threadIdx.x; f < kCfTriples * C::LPR; f += C::THREADS) {
    const int k = f / C::LPR, c = f % C::LPR;
    const bool ok = k < n_tr && 4 * c < in.d;
    f32x4 v = ld4(in.U + (ok ? static_cast<int64_t>(sh_user[k]) * in.ldu + 4 * c : 0));
    if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(An + (k * C::LDF + 4 * c) * 4) = v;
  }
}

template <int KQ>
struct CF {
  using C = VA<KQ>;
  static constexpr size_t AN_BYTES = static_cast<size_t>(kCfTriples) * C::LDF * 4;
  static constexpr size_t LDS_FWD = C::LDS_FWD + AN_BYTES;
  static constexpr size_t LDS_BWD = C::LDS_BWD + AN_BYTES;
};

// ---- forward (attention) --------------------------------------------------------------------
// k_va_forward's two phases on the gathered rows; F replaces z0 in LDS (a lane's piece of z0 is
// read by that lane alone). Then a wave per triple: lanes 0-31 hold the positive row's float4
// pieces, lanes 32-63 the negative's; ⟨a, F⟩, ‖F‖², ‖a‖² as fmaf chains and a 32-lane butterfly.
template <int KQ>
__global__ __launch_bounds__(VA<KQ>::THREADS) void k_cf_forward(CfFwd p) {
  using C = VA<KQ>;
  extern __shared__ __align__(16) char va_smem[];
  __shared__ int sh_item[kVaRows], sh_user[kCfTriples];
  __shared__ float sh_red[kCfTriples][kCfPart];
  char* Zp = va_smem + 2 * C::F32_BYTES;  // [2 views][3][plane]
  char* Dp = Zp + 2 * C::OPER_BYTES;      // t_0 − t_1
  char* An = Dp + C::OPER_BYTES;          // the anchors
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int ct = wave % C::NCT, rt0 = wave / C::NCT;
  const int col0 = 16 * ct + 4 * g;
  const bool live = 16 * ct < p.in.d;

  bf16x8 w1[KQ][3], w2[KQ][3];
  load_wfrag<KQ>(p.in.W1, p.in.d, 1, p.in.d, 16 * ct + i16, g, w1);  // Bm[k][n] = W1[n][k]
  load_wfrag<KQ>(p.in.W2, p.in.d, 1, p.in.d, 16 * ct + i16, g, w2);
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (live) bias = f32x4{p.in.b1[col0], p.in.b1[col0 + 1], p.in.b1[col0 + 2], p.in.b1[col0 + 3]};

  const int64_t nblocks = (p.in.B + kCfTriples - 1) / kCfTriples;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t t0 = blk * kCfTriples, r0 = 2 * t0;
    const int n_tr = static_cast<int>(std::min<int64_t>(kCfTriples, p.in.B - t0));
    __syncthreads();  // the previous block's rows, planes and sums are read
    block_ids(p.in, t0, n_tr, sh_item, sh_user);
    __syncthreads();
    {
      f32x4 v[Stage<KQ, 2>::F];
      load_views<KQ>(p.in, sh_item, 2 * n_tr, v);
      store_block<KQ, 2>(v, va_smem, Zp);
    }
    stage_anchors<KQ>(p.in, sh_user, n_tr, An);
    __syncthreads();
#pragma unroll
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const f32x4 t0v = tanh4(tile_product<KQ>(Zp, rt, i16, g, w1) + bias);
      const f32x4 t1v = tanh4(tile_product<KQ>(Zp + C::OPER_BYTES, rt, i16, g, w1) + bias);
      put_planes<KQ>(Dp, 16 * rt + i16, 4 * ct + g, t0v - t1v);  // a dead tile: exact zeros
    }
    __syncthreads();
#pragma unroll
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const f32x4 q = tile_product<KQ>(Dp, rt, i16, g, w2);
      const int rl = 16 * rt + i16;
      f32x4* z0p = reinterpret_cast<f32x4*>(va_smem + (rl * C::LDF + col0) * 4);
      const f32x4 z0 = *z0p;
      const f32x4 z1 =
          *reinterpret_cast<const f32x4*>(va_smem + C::F32_BYTES + (rl * C::LDF + col0) * 4);
      f32x4 b0, o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        b0[j] = sigmoid_stable(q[j]);
        o[j] = fmaf(b0[j], z0[j], (1.f - b0[j]) * z1[j]);
      }
      *z0p = o;  // F: zeros in a dead tile and past the batch's end
      if (p.beta0 && live && rl < 2 * n_tr)
        *reinterpret_cast<f32x4*>(p.beta0 + (r0 + rl) * p.ldb + col0) = b0;
    }
    __syncthreads();  // F is whole
    {
      const int half = lane >> 5, c = lane & 31;
      for (int k = wave; k < kCfTriples; k += C::THREADS / 64) {
        float dot = 0.f, sf = 0.f, sa = 0.f;
        if (c < C::LPR) {
          const f32x4 f =
              *reinterpret_cast<const f32x4*>(va_smem + ((2 * k + half) * C::LDF + 4 * c) * 4);
          const f32x4 a = *reinterpret_cast<const f32x4*>(An + (k * C::LDF + 4 * c) * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            dot = fmaf(a[j], f[j], dot);
            sf = fmaf(f[j], f[j], sf);
            sa = fmaf(a[j], a[j], sa);
          }
        }
        dot = group_sum<32>(dot);
        sf = group_sum<32>(sf);
        sa = group_sum<32>(sa);
        const float dot_n = __shfl(dot, 32), sf_n = __shfl(sf, 32);
        if (lane == 0) {
          float l = 0.f, cf = 0.f;
          if (k < n_tr) {
            bpr_terms(dot - dot_n, l, cf);
            p.coef[t0 + k] = cf;
          }
          sh_red[k][0] = l;
          sh_red[k][1] = sa;
          sh_red[k][2] = sf;
          sh_red[k][3] = sf_n;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < kCfPart) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < kCfTriples; ++k) s += sh_red[k][threadIdx.x];
      p.part[blk * kCfPart + threadIdx.x] = s;
    }
  }
}

// ---- backward (attention) -------------------------------------------------------------------
// Phase 0: F = β0 ⊙ z0 + (1 − β0) ⊙ z1 again (the forward's expression), dF → the LDS rows
// k_va_backward stages dOut into, da_k → DA. Phases A-C: k_va_backward on those rows.
template <int KQ>
__global__ __launch_bounds__(VA<KQ>::THREADS) void k_cf_backward(CfBwd p) {
  using C = VA<KQ>;
  extern __shared__ __align__(16) char va_smem[];
  __shared__ int sh_item[kVaRows], sh_user[kCfTriples];
  __shared__ CfScale sh_scale;  // (in LDS: live in registers for phase 0 alone)
  char* Zp = va_smem + 4 * C::F32_BYTES;  // [2][3][plane]: the views, then da_0 / da_1
  char* Dp = Zp + 2 * C::OPER_BYTES;      // dq
  char* An = Dp + C::OPER_BYTES;          // the anchors
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int ct = wave % C::NCT, rt0 = wave / C::NCT;
  const int col0 = 16 * ct + 4 * g;
  const int d = p.in.d;
  const bool live = 16 * ct < d;
  const bool want_rows = p.dz[0] != nullptr;

  bf16x8 w1[KQ][3], w2t[KQ][3], w1t[KQ][3];
  load_wfrag<KQ>(p.in.W1, d, 1, d, 16 * ct + i16, g, w1);   // Bm[k][n] = W1[n][k]
  load_wfrag<KQ>(p.in.W2, d, d, 1, 16 * ct + i16, g, w2t);  // Bm[k][n] = W2[k][n]
  load_wfrag<KQ>(p.in.W1, d, d, 1, 16 * ct + i16, g, w1t);  // Bm[k][n] = W1[k][n]
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (live) bias = f32x4{p.in.b1[col0], p.in.b1[col0 + 1], p.in.b1[col0 + 2], p.in.b1[col0 + 3]};
  if (threadIdx.x == 0) sh_scale = load_scale(p);  // (the loop's first barriers publish it)

  const int64_t nblocks = (p.in.B + kCfTriples - 1) / kCfTriples;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t t0 = blk * kCfTriples, r0 = 2 * t0;
    const int n_tr = static_cast<int>(std::min<int64_t>(kCfTriples, p.in.B - t0));
    const int n_pos = 2 * n_tr;
    __syncthreads();  // the previous block's rows and planes are read
    block_ids(p.in, t0, n_tr, sh_item, sh_user);
    __syncthreads();
    {
      f32x4 v[Stage<KQ, 2>::F];
      load_views<KQ>(p.in, sh_item, n_pos, v);
      store_block<KQ, 2>(v, va_smem, Zp);
      if (p.ops) {  // the views' rows as the split-K products read them
        using S = Stage<KQ, 2>;
#pragma unroll
        for (int u = 0; u < S::F; ++u) {
          const int f = threadIdx.x + C::THREADS * u;
          const int a = f / S::PER, rem = f % S::PER;
          const int rl = rem / C::LPR, c = rem % C::LPR;
          if (rl < n_pos && 4 * c < d)
            *reinterpret_cast<f32x4*>(p.ops + (4 + a) * p.op_stride + (r0 + rl) * d + 4 * c) =
                v[u];
        }
      }
    }
#pragma unroll 1
    for (int f = threadIdx.x; f < kVaRows * C::LPR; f += C::THREADS) {
      const int rl = f / C::LPR, c = f % C::LPR;
      const bool ok = rl < n_pos && 4 * c < d;
      f32x4 v = ld4(p.beta0 + (ok ? (r0 + rl) * p.ldb + 4 * c : 0));
      if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(va_smem + 3 * C::F32_BYTES + (rl * C::LDF + 4 * c) * 4) = v;
    }
    stage_anchors<KQ>(p.in, sh_user, n_tr, An);
    __syncthreads();
#pragma unroll 1
    for (int f = threadIdx.x; f < kCfTriples * C::LPR; f += C::THREADS) {
      const CfScale sc = sh_scale;
      const int k = f / C::LPR, c = f % C::LPR;
      const int at = (2 * k * C::LDF + 4 * c) * 4, nx = C::LDF * 4;  // the positive row, + nx
      const f32x4 z0p = *reinterpret_cast<const f32x4*>(va_smem + at);
      const f32x4 z0n = *reinterpret_cast<const f32x4*>(va_smem + at + nx);
      const f32x4 z1p = *reinterpret_cast<const f32x4*>(va_smem + C::F32_BYTES + at);
      const f32x4 z1n = *reinterpret_cast<const f32x4*>(va_smem + C::F32_BYTES + at + nx);
      const f32x4 bp = *reinterpret_cast<const f32x4*>(va_smem + 3 * C::F32_BYTES + at);
      const f32x4 bn = *reinterpret_cast<const f32x4*>(va_smem + 3 * C::F32_BYTES + at + nx);
      const f32x4 a = *reinterpret_cast<const f32x4*>(An + (k * C::LDF + 4 * c) * 4);
      const float ck = k < n_tr ? sc.gB * p.coef[t0 + k] : 0.f;
      f32x4 gp, gn, da;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float fp = fmaf(bp[j], z0p[j], (1.f - bp[j]) * z1p[j]);
        const float fn = fmaf(bn[j], z0n[j], (1.f - bn[j]) * z1n[j]);
        gp[j] = fmaf(-ck, a[j], sc.sP * fp);
        gn[j] = fmaf(ck, a[j], sc.sN * fn);
        da[j] = fmaf(-ck, fp - fn, sc.sA * a[j]);
      }
      *reinterpret_cast<f32x4*>(va_smem + 2 * C::F32_BYTES + at) = gp;
      *reinterpret_cast<f32x4*>(va_smem + 2 * C::F32_BYTES + at + nx) = gn;
      if (p.dA && k < n_tr && 4 * c < d)
        *reinterpret_cast<f32x4*>(p.dA + (t0 + k) * p.ldda + 4 * c) = da;
    }
    if (!want_rows && !p.ops) continue;  // (uniform) the anchors' gradient alone
    __syncthreads();  // dF is whole
    // (the row-tile loops stay rolled, as in k_va_backward)
#pragma unroll 1
    for (int ri = 0; ri < C::RI; ++ri) {
      const int rt = rt0 + ri * C::RTW;
      const int rl = 16 * rt + i16;
      const f32x4 t0v = tanh4(tile_product<KQ>(Zp, rt, i16, g, w1) + bias);
      const f32x4 t1v = tanh4(tile_product<KQ>(Zp + C::OPER_BYTES, rt, i16, g, w1) + bias);
      const int at = (rl * C::LDF + col0) * 4;
      f32x4* z0p = reinterpret_cast<f32x4*>(va_smem + at);
      f32x4* z1p = reinterpret_cast<f32x4*>(va_smem + C::F32_BYTES + at);
      const f32x4 gg = *reinterpret_cast<const f32x4*>(va_smem + 2 * C::F32_BYTES + at);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(va_smem + 3 * C::F32_BYTES + at);
      const f32x4 dq = gg * (*z0p - *z1p) * (b0 * (1.f - b0));
      *z0p = 1.f - t0v * t0v;
      *z1p = 1.f - t1v * t1v;
      put_planes<KQ>(Dp, rl, 4 * ct + g, dq);
      if (p.ops && live && rl < n_pos) {
        float* o = p.ops + (r0 + rl) * d + col0;
        *reinterpret_cast<f32x4*>(o) = dq;
        *reinterpret_cast<f32x4*>(o + p.op_stride) = t0v - t1v;
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
      if (p.ops && live && rl < n_pos) {
        float* o = p.ops + 2 * p.op_stride + (r0 + rl) * d + col0;
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
      if (live && rl < n_pos) {
        *reinterpret_cast<f32x4*>(p.dz[0] + (r0 + rl) * p.lddz[0] + col0) = d0;
        *reinterpret_cast<f32x4*>(p.dz[1] + (r0 + rl) * p.lddz[1] + col0) = d1;
      }
    }
  }
}

// ---- mean mode ------------------------------------------------------------------------------
// F = (z0 + z1)/2: no products, nothing staged. A workgroup of four waves owns the same 16
// triples; a wave takes a triple at a time, lanes 0-31 the positive row's float4 pieces (32 apart
// when d > 128), lanes 32-63 the negative's.
constexpr int kMeanWaves = kBlock / 64;

__global__ __launch_bounds__(kBlock) void k_cf_mean_forward(CfIn in, float* __restrict__ coef,
                                                            float* __restrict__ part) {
  __shared__ float sh_red[kCfTriples][kCfPart];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, c0 = lane & 31;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kCfTriples;
  for (int k = wave; k < kCfTriples; k += kMeanWaves) {
    const int64_t t = t0 + k;
    const bool valid = t < in.B;  // (uniform in the wave)
    float dot = 0.f, sf = 0.f, sa = 0.f;
    if (valid) {
      const int64_t item = half ? in.nid[t] : in.pid[t];
      const float* z0 = in.z[0] + item * in.ld[0];
      const float* z1 = in.z[1] + item * in.ld[1];
      const float* u = in.U + static_cast<int64_t>(in.uid[t]) * in.ldu;
      for (int c = c0; 4 * c < in.d; c += 32) {
        const f32x4 f = (ld4(z0 + 4 * c) + ld4(z1 + 4 * c)) * 0.5f;
        const f32x4 a = ld4(u + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dot = fmaf(a[j], f[j], dot);
          sf = fmaf(f[j], f[j], sf);
          sa = fmaf(a[j], a[j], sa);
        }
      }
    }
    dot = group_sum<32>(dot);
    sf = group_sum<32>(sf);
    sa = group_sum<32>(sa);
    const float dot_n = __shfl(dot, 32), sf_n = __shfl(sf, 32);
    if (lane == 0) {
      float l = 0.f, cf = 0.f;
      if (valid) {
        bpr_terms(dot - dot_n, l, cf);
        coef[t] = cf;
      }
      sh_red[k][0] = l;
      sh_red[k][1] = sa;
      sh_red[k][2] = sf;
      sh_red[k][3] = sf_n;
    }
  }
  __syncthreads();
  if (threadIdx.x < kCfPart) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kCfTriples; ++k) s += sh_red[k][threadIdx.x];
    part[static_cast<int64_t>(blockIdx.x) * kCfPart + threadIdx.x] = s;
  }
}

// dZ0 = dZ1 = dF/2 per position, DA per triple (the other half's F through a lane exchange)
__global__ __launch_bounds__(kBlock) void k_cf_mean_backward(CfBwd p) {
  const CfIn& in = p.in;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, c0 = lane & 31;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kCfTriples;
  const CfScale sc = load_scale(p);
  for (int k = wave; k < kCfTriples; k += kMeanWaves) {
    const int64_t t = t0 + k;
    if (t >= in.B) break;  // (uniform in the wave)
    const int64_t item = half ? in.nid[t] : in.pid[t];
    const float* z0 = in.z[0] + item * in.ld[0];
    const float* z1 = in.z[1] + item * in.ld[1];
    const float* u = in.U + static_cast<int64_t>(in.uid[t]) * in.ldu;
    const float ck = sc.gB * p.coef[t];
    const float sgn = half ? ck : -ck, sF = half ? sc.sN : sc.sP;
    for (int cb = 0; 4 * cb < in.d; cb += 32) {  // (uniform: the exchange needs every lane)
      const int c = cb + c0;
      const bool ok = 4 * c < in.d;
      f32x4 f = {0.f, 0.f, 0.f, 0.f}, a = f, fo;
      if (ok) {
        f = (ld4(z0 + 4 * c) + ld4(z1 + 4 * c)) * 0.5f;
        a = ld4(u + 4 * c);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) fo[j] = __shfl_xor(f[j], 32);
      if (!ok) continue;
      if (p.dz[0]) {
        f32x4 dh;
#pragma unroll
        for (int j = 0; j < 4; ++j) dh[j] = 0.5f * fmaf(sgn, a[j], sF * f[j]);
        *reinterpret_cast<f32x4*>(p.dz[0] + (2 * t + half) * p.lddz[0] + 4 * c) = dh;
        *reinterpret_cast<f32x4*>(p.dz[1] + (2 * t + half) * p.lddz[1] + 4 * c) = dh;
      }
      if (p.dA && half == 0) {
        f32x4 da;
#pragma unroll
        for (int j = 0; j < 4; ++j) da[j] = fmaf(-ck, f[j] - fo[j], sc.sA * a[j]);
        *reinterpret_cast<f32x4*>(p.dA + t * p.ldda + 4 * c) = da;
      }
    }
  }
}

// The second stage: the blocks' partials in block order per thread, then a fixed tree.
//   norms = (‖A‖, ‖P‖, ‖N‖);  loss = Σℓ / B + reg · (Σ norms) / batch_size
__global__ __launch_bounds__(kBlock) void k_cf_finish(const float* __restrict__ part,
                                                      int64_t n_blocks, float fB, float reg,
                                                      float bs, float* __restrict__ norms,
                                                      float* __restrict__ loss) {
  __shared__ float sh[kCfPart][kBlock];
  float s[kCfPart] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t t = threadIdx.x; t < n_blocks; t += kBlock) {
#pragma unroll
    for (int q = 0; q < kCfPart; ++q) s[q] += part[t * kCfPart + q];
  }
#pragma unroll
  for (int q = 0; q < kCfPart; ++q) sh[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int m = kBlock / 2; m >= 1; m >>= 1) {
    if (static_cast<int>(threadIdx.x) < m) {
#pragma unroll
      for (int q = 0; q < kCfPart; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + m];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float total = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float nq = sqrtf(sh[1 + q][0]);
      norms[q] = nq;
      total += nq;
    }
    loss[0] = sh[0][0] / fB + total * reg / bs;
  }
}

template <int KQ>
hgd_status launch_forward(const CfFwd& p, int64_t nblocks, hipStream_t st, const char* fn) {
  using C = VA<KQ>;
  static int resident[kMaxDevices] = {};
  int cap = 0;
  if (hgd_status s =
          resident_blocks(k_cf_forward<KQ>, C::THREADS, CF<KQ>::LDS_FWD, resident, &cap))
    return s;
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>(nblocks, cap));
  hipLaunchKernelGGL(k_cf_forward<KQ>, dim3(grid), dim3(C::THREADS), CF<KQ>::LDS_FWD, st, p);
  return check_launch(fn);
}

template <int KQ>
hgd_status launch_backward(const CfBwd& p, int64_t nblocks, hipStream_t st, const char* fn) {
  using C = VA<KQ>;
  static int resident[kMaxDevices] = {};
  int cap = 0;
  if (hgd_status s =
          resident_blocks(k_cf_backward<KQ>, C::THREADS, CF<KQ>::LDS_BWD, resident, &cap))
    return s;
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>(nblocks, cap));
  hipLaunchKernelGGL(k_cf_backward<KQ>, dim3(grid), dim3(C::THREADS), CF<KQ>::LDS_BWD, st, p);
  return check_launch(fn);
}

bool attention_width(int32_t d) { return d >= 16 && d <= 128 && d % 16 == 0; }
bool mean_width(int32_t d) { return d >= 4 && d <= 256 && d % 4 == 0; }

int64_t cf_blocks(int64_t B) { return (B + kCfTriples - 1) / kCfTriples; }
size_t part_bytes(int64_t B) {
  return align_up(static_cast<size_t>(cf_blocks(B)) * kCfPart * sizeof(float));
}

// The parameter path's workspace behind the forward's partials: the six operands, the second
// view's dW1 / db1 terms, and hgd_gemm_tn's split-K partials (the larger of the two calls).
struct ParamPlan {
  size_t op_bytes, tmp_bytes, tn_bytes;
  hgd_gemm_tn_desc w1[2], w2;
  size_t total() const { return 6 * op_bytes + tmp_bytes + tn_bytes; }
};

ParamPlan param_plan(int64_t B, int32_t d, char* ws, float* dW1, float* db1, float* dW2) {
  ParamPlan pl{};
  const int64_t n = 2 * B;
  pl.op_bytes = align_up(static_cast<size_t>(n) * d * sizeof(float));
  pl.tmp_bytes = align_up((static_cast<size_t>(d) * d + d) * sizeof(float));
  float* ops = reinterpret_cast<float*>(ws);
  const size_t stride = pl.op_bytes / sizeof(float);
  float* tmp = reinterpret_cast<float*>(ws + 6 * pl.op_bytes);
  for (int v = 0; v < 2; ++v) {
    hgd_gemm_tn_desc& e = pl.w1[v];
    e.A = ops + (2 + v) * stride;  // da_v
    e.lda = d;
    e.B = ops + (4 + v) * stride;  // z_v at the positions
    e.ldb = d;
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

hgd_status check_common(const char* fn, const float* U, int64_t ldu, const int32_t* uid,
                        int64_t n_users, const float* Z0, int64_t ld0, const float* Z1,
                        int64_t ld1, const int32_t* pid, const int32_t* nid, int64_t n_items,
                        int64_t batch, int32_t d, const float* W1, const float* b1,
                        const float* W2, int64_t batch_size, bool* attention) {
  const bool att = W1 != nullptr;
  HGD_REQUIRE(att == (b1 != nullptr) && att == (W2 != nullptr),
              "%s: W1, b1 and W2 go together (all NULL = the mean of the views)", fn);
  if (att)
    HGD_REQUIRE(attention_width(d),
                "%s: d = %d is not a fused width (a multiple of 16 in [16, 128])", fn, d);
  else
    HGD_REQUIRE(mean_width(d),
                "%s: d = %d is not a mean-mode width (a multiple of 4 in [4, 256])", fn, d);
  HGD_REQUIRE(batch >= 0 && batch < (int64_t{1} << 30), "%s: batch out of range", fn);
  HGD_REQUIRE(n_users > 0 && n_users < 0x7fffffffLL && n_items > 0 && n_items < 0x7fffffffLL,
              "%s: n_users / n_items out of range", fn);
  HGD_REQUIRE(batch_size > 0, "%s: batch_size must be > 0", fn);
  HGD_REQUIRE(ldu >= d && ld0 >= d && ld1 >= d, "%s: the rows' leading dimensions must be >= d",
              fn);
  HGD_REQUIRE(U && uid && Z0 && Z1 && pid && nid, "%s: null pointer", fn);
  HGD_REQUIRE(al16r(U, ldu) && al16r(Z0, ld0) && al16r(Z1, ld1),
              "%s: the rows of U / Z0 / Z1 must be 16-byte aligned", fn);
  *attention = att;
  return HGD_OK;
}

}  // namespace
}  // namespace hgd

using namespace hgd;

extern "C" size_t hgd_cf_loss_workspace_size(int64_t batch, int32_t d, int32_t with_params) {
  if (batch <= 0 || batch >= (int64_t{1} << 30)) return 0;
  if (with_params ? !attention_width(d) : !mean_width(d)) return 0;
  size_t total = part_bytes(batch);
  if (with_params) {
    // placeholders with the alignment the calls require: only sizes are read
    float* const a16 = reinterpret_cast<float*>(uintptr_t{256});
    total += param_plan(batch, d, reinterpret_cast<char*>(a16), a16, a16, a16).total();
  }
  return total;
}

extern "C" hgd_status hgd_cf_loss_forward(
    const float* U, int64_t ldu, const int32_t* uid, int64_t n_users, const float* Z0,
    int64_t ld0, const float* Z1, int64_t ld1, const int32_t* pid, const int32_t* nid,
    int64_t n_items, int64_t batch, int32_t d, const float* W1, const float* b1, const float* W2,
    float reg, int64_t batch_size, float* beta0, int64_t ldb, float* coef, float* norms,
    float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  const char* fn = "hgd_cf_loss_forward";
  bool att = false;
  if (hgd_status st = check_common(fn, U, ldu, uid, n_users, Z0, ld0, Z1, ld1, pid, nid, n_items,
                                   batch, d, W1, b1, W2, batch_size, &att))
    return st;
  HGD_REQUIRE(coef && norms && loss, "%s: null pointer", fn);
  HGD_REQUIRE(!beta0 || att, "%s: beta0 belongs to the attention mode", fn);
  HGD_REQUIRE(!beta0 || ldb >= d, "%s: ldb must be >= d", fn);
  HGD_REQUIRE(!beta0 || al16r(beta0, ldb), "%s: the rows of beta0 must be 16-byte aligned", fn);
  if (batch == 0) return HGD_OK;
  const size_t need = part_bytes(batch);
  HGD_REQUIRE(al16p(workspace), "%s: misaligned workspace", fn);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", fn,
                workspace == nullptr ? size_t{0} : workspace_bytes, need);
  const CfIn in{U, ldu, uid, {Z0, Z1}, {ld0, ld1}, pid, nid, batch, d, W1, b1, W2};
  float* part = static_cast<float*>(workspace);
  const int64_t nblocks = cf_blocks(batch);
  hipStream_t st = as_stream(stream);
  hgd_status ls;
  if (att) {
    const CfFwd p{in, beta0, ldb, coef, part};
    switch ((d + 31) / 32) {
      case 1: ls = launch_forward<1>(p, nblocks, st, fn); break;
      case 2: ls = launch_forward<2>(p, nblocks, st, fn); break;
      case 3: ls = launch_forward<3>(p, nblocks, st, fn); break;
      default: ls = launch_forward<4>(p, nblocks, st, fn); break;
    }
  } else {
    hipLaunchKernelGGL(k_cf_mean_forward, dim3(static_cast<unsigned>(nblocks)), dim3(kBlock), 0,
                       st, in, coef, part);
    ls = check_launch(fn);
  }
  if (ls != HGD_OK) return ls;
  hipLaunchKernelGGL(k_cf_finish, dim3(1), dim3(kBlock), 0, st, part, nblocks,
                     static_cast<float>(batch), reg, static_cast<float>(batch_size), norms, loss);
  return check_launch(fn);
}

extern "C" hgd_status hgd_cf_loss_backward(
    const float* U, int64_t ldu, const int32_t* uid, int64_t n_users, const float* Z0,
    int64_t ld0, const float* Z1, int64_t ld1, const int32_t* pid, const int32_t* nid,
    int64_t n_items, int64_t batch, int32_t d, const float* W1, const float* b1, const float* W2,
    float reg, int64_t batch_size, const float* beta0, int64_t ldb, const float* coef,
    const float* norms, const float* grad, float* dA, int64_t ldda, float* dZ0, int64_t lddz0,
    float* dZ1, int64_t lddz1, float* dW1, float* db1, float* dW2, void* workspace,
    size_t workspace_bytes, void* stream) {
  clear_error();
  const char* fn = "hgd_cf_loss_backward";
  bool att = false;
  if (hgd_status st = check_common(fn, U, ldu, uid, n_users, Z0, ld0, Z1, ld1, pid, nid, n_items,
                                   batch, d, W1, b1, W2, batch_size, &att))
    return st;
  HGD_REQUIRE(coef && norms && grad && (!att || beta0), "%s: null pointer", fn);
  HGD_REQUIRE(!att || ldb >= d, "%s: ldb must be >= d", fn);
  HGD_REQUIRE(!att || al16r(beta0, ldb), "%s: the rows of beta0 must be 16-byte aligned", fn);
  HGD_REQUIRE(!dA || ldda >= d, "%s: ldda must be >= d", fn);
  HGD_REQUIRE(!dA || al16r(dA, ldda), "%s: the rows of dA must be 16-byte aligned", fn);
  HGD_REQUIRE((dZ0 == nullptr) == (dZ1 == nullptr), "%s: dZ0 and dZ1 go together", fn);
  HGD_REQUIRE(!dZ0 || (lddz0 >= d && lddz1 >= d), "%s: lddz0 / lddz1 must be >= d", fn);
  HGD_REQUIRE(!dZ0 || (al16r(dZ0, lddz0) && al16r(dZ1, lddz1)),
              "%s: the rows of dZ0 / dZ1 must be 16-byte aligned", fn);
  const bool params = dW1 != nullptr;
  HGD_REQUIRE(params == (db1 != nullptr) && params == (dW2 != nullptr),
              "%s: dW1, db1 and dW2 go together", fn);
  HGD_REQUIRE(!params || att, "%s: the mean of the views has no parameters", fn);
  HGD_REQUIRE(dA || dZ0 || params, "%s: nothing to compute (no dA, no dZ, no parameter gradients)",
              fn);
  if (batch == 0) return HGD_OK;
  ParamPlan pl{};
  char* pws = nullptr;
  if (params) {
    const size_t need = hgd_cf_loss_workspace_size(batch, d, 1);
    HGD_REQUIRE(al16p(workspace), "%s: misaligned workspace", fn);
    if (workspace == nullptr || workspace_bytes < need)
      return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", fn,
                  workspace == nullptr ? size_t{0} : workspace_bytes, need);
    pws = static_cast<char*>(workspace) + part_bytes(batch);
    pl = param_plan(batch, d, pws, dW1, db1, dW2);
  }
  const CfIn in{U, ldu, uid, {Z0, Z1}, {ld0, ld1}, pid, nid, batch, d, W1, b1, W2};
  CfBwd p{in, beta0, ldb, coef, norms, grad, reg / static_cast<float>(batch_size), dA, ldda,
          {dZ0, dZ1}, {lddz0, lddz1}, nullptr, 0};
  if (params) {
    p.ops = reinterpret_cast<float*>(pws);
    p.op_stride = static_cast<int64_t>(pl.op_bytes / sizeof(float));
  }
  const int64_t nblocks = cf_blocks(batch);
  hipStream_t st = as_stream(stream);
  if (!att) {
    hipLaunchKernelGGL(k_cf_mean_backward, dim3(static_cast<unsigned>(nblocks)), dim3(kBlock), 0,
                       st, p);
    return check_launch(fn);
  }
  hgd_status ls;
  switch ((d + 31) / 32) {
    case 1: ls = launch_backward<1>(p, nblocks, st, fn); break;
    case 2: ls = launch_backward<2>(p, nblocks, st, fn); break;
    case 3: ls = launch_backward<3>(p, nblocks, st, fn); break;
    default: ls = launch_backward<4>(p, nblocks, st, fn); break;
  }
  if (ls != HGD_OK || !params) return ls;
  // dW1 = da_0ᵀ·z0 + da_1ᵀ·z1, db1 = Σ_positions (da_0 + da_1), dW2 = dqᵀ·(t_0 − t_1), as
  // hgd_view_attention_backward reduces them
  char* tn_ws = pws + 6 * pl.op_bytes + pl.tmp_bytes;
  if (hgd_status s = hgd_gemm_tn(pl.w1, 2, tn_ws, pl.tn_bytes, stream)) return s;
  const int nW = d * d;
  hipLaunchKernelGGL(k_va_add, dim3(grid_for(nW + d)), dim3(kBlock), 0, st, dW1, pl.w1[1].C, nW,
                     db1, pl.w1[1].colsum_A, d);
  if (hgd_status s = check_launch(fn)) return s;
  return hgd_gemm_tn(&pl.w2, 1, tn_ws, pl.tn_bytes, stream);
}
