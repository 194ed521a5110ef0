// KHGRec's TransR knowledge-graph loss on the device (include/hgd.h, "KG loss"):
//   hgd_kg_loss_forward   calculate_kg_loss (KHGRec.py:347-365) for a whole batch of triples
//   hgd_kg_loss_backward  its gradients: the rows' [3B, d], trans_M's and relation_emb's in full
// The reference gathers W_r = trans_M[r] per triple ([B, d, dr]) and reads it in three bmm calls;
// here a workgroup owns kTile consecutive triples of ONE relation in the relation-grouped order
// (kg_tile.h) and reads that relation's W_r once. fp32, every sum in a fixed order, no atomics:
// two runs are bitwise equal.
#include <cmath>

#include "device_util.h"
#include "hgd_internal.h"
#include "kg_tile.h"

namespace hgd {
namespace {

// Thread (slot, lane) as in k_kg_scores: lane = a column of a 32-wide pass, slot = kTT of the
// tile's triples. The staged chunk of the three gathered rows is kJC = 64 columns (k_kg_scores
// stages two rows at 128): 24 KB, which leaves up to kWLdsMax for W_r inside the 64 KB a
// workgroup gets without asking for more, so (d, dr) = (128, 64) still reads W_r from LDS.
constexpr int kTile = kKgTile;
constexpr int kKC = 32;
constexpr int kJC = 64;
constexpr int kGC = 64;  // relation-space columns of one chunk of the backward's gradients
constexpr int kSlots = kBlock / kKC;
constexpr int kTT = kTile / kSlots;
constexpr int kStage = 4;  // staged elements per thread and row kind whose loads overlap
constexpr size_t kWLdsMax = 36 * 1024;
constexpr int kPart = 8;  // floats of a tile's partial sums (5 used)

static_assert(kSlots * kTT == kTile && kKC == 32 && kJC == 2 * kKC && kGC == 2 * kKC &&
                  kJC == kSlots * 8,
              "tile geometry");

// The three row sources (h, pos_t, neg_t): row i of kind s is x[s] + (idx[s] ? idx[s][i] : i)·ld[s]
struct Rows {
  const float* x[3];
  int64_t ld[3];
  const int32_t* idx[3];
};

// the tile's row numbers per kind (slots past the tile's end: row 0, never stored)
__device__ __forceinline__ void tile_rows(const Rows& rows, const int32_t* __restrict__ grp_perm,
                                          int base, int n_here, int (*sh_row)[kTile],
                                          int* sh_id) {
  if (threadIdx.x < kTile) {
    const int i = threadIdx.x;
    const int id = i < n_here ? grp_perm[base + i] : 0;
    if (sh_id) sh_id[i] = id;
    if (sh_row) {
#pragma unroll
      for (int s = 0; s < 3; ++s)
        sh_row[s][i] = (i < n_here && rows.idx[s] != nullptr) ? rows.idx[s][id] : id;
    }
  }
}

// Xs[s][i][0 .. kJC) = columns [j0, j0 + kJC) of the tile's rows, zeros past column d and for the
// slots past n_rows; kStage elements of every kind per thread in flight before the first store
__device__ __forceinline__ void stage_rows(const Rows& rows, const int (*sh_row)[kTile],
                                           int n_rows, int j0, int d, int width,
                                           float* __restrict__ Xs) {
  const int total = kTile * width;
  for (int e0 = threadIdx.x; e0 < total; e0 += kBlock * kStage) {
    float v[3][kStage];
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int e = e0 + u * kBlock;
      v[0][u] = v[1][u] = v[2][u] = 0.f;
      if (e < total) {
        const int i = e / width, j = e - i * width;
        if (i < n_rows && j0 + j < d) {
#pragma unroll
          for (int s = 0; s < 3; ++s)
            v[s][u] = rows.x[s][static_cast<int64_t>(sh_row[s][i]) * rows.ld[s] + j0 + j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int e = e0 + u * kBlock;
      if (e < total) {
        const int i = e / width, j = e - i * width;
#pragma unroll
        for (int s = 0; s < 3; ++s) Xs[(s * kTile + i) * kJC + j] = v[s][u];
      }
    }
  }
}

// ---- forward --------------------------------------------------------------------------------
// Per relation-space pass of 32 columns: a, p, n of the slot's kTT triples as fmaf chains over
// the embedding columns in ascending order; the projections are saved in GROUPED order
// (proj[s][position][k]), the squared distances are a per-lane chain over the passes and a
// 32-lane butterfly. The tile's five sums (Σ softplus, Σ a², Σ e², Σ p², Σ n²) go to part[tile].
template <bool W_LDS>
__global__ __launch_bounds__(kBlock) void k_kgl_forward(
    Rows rows, const float* __restrict__ W, const float* __restrict__ R, int64_t ldR, int n_rel,
    int d, int dr, const int32_t* __restrict__ grp_perm, const int64_t* __restrict__ rel_off,
    int B, float* __restrict__ proj, float* __restrict__ coef, float* __restrict__ part) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int sh_row[3][kTile];
  __shared__ float red[kSlots][kPart];
  float* Xs = smem;
  float* Ws = smem + 3 * kTile * kJC;

  const uint8_t* const all_relations = nullptr;
  HGD_KG_FIND_TILE(n_rel, rel_off, all_relations, rel, base, end);
  if (rel < 0) {
    // a surplus workgroup: its partial is part of the second stage's sum
    if (threadIdx.x < kPart) part[static_cast<int64_t>(blockIdx.x) * kPart + threadIdx.x] = 0.f;
    return;
  }
  const int n_here = min(kTile, end - base);
  tile_rows(rows, grp_perm, base, n_here, sh_row, nullptr);
  const float* Wr = W + static_cast<int64_t>(rel) * d * dr;
  const int dP = (d + 3) & ~3;
  if constexpr (W_LDS) {
    for (int idx = threadIdx.x; idx < dP * dr; idx += kBlock)
      Ws[idx] = idx < d * dr ? Wr[idx] : 0.f;
  }

  const int lane = threadIdx.x & (kKC - 1);
  const int slot = threadIdx.x / kKC;
  const int n_jc = (d + kJC - 1) / kJC;
  const float fB = static_cast<float>(B);
  float dpos[kTT], dneg[kTT], sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < kTT; ++u) dpos[u] = dneg[u] = 0.f;

  for (int k0 = 0; k0 < dr; k0 += kKC) {
    const int k = k0 + lane;
    const bool kvalid = k < dr;
    float pa[kTT], pp[kTT], pn[kTT];
#pragma unroll
    for (int u = 0; u < kTT; ++u) pa[u] = pp[u] = pn[u] = 0.f;
    for (int jc = 0; jc < n_jc; ++jc) {
      const int j0 = jc * kJC;
      const int jn = min(kJC, d - j0);
      const int jnP = (jn + 3) & ~3;
      __syncthreads();  // the rows and W_r are written; the previous chunk's rows are read
      if (n_jc > 1 || k0 == 0) stage_rows(rows, sh_row, kTile, j0, d, jnP, Xs);
      __syncthreads();
      for (int j = 0; j < jnP; j += 4) {
        float w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jj = j0 + j + q;
          if constexpr (W_LDS)
            w[q] = kvalid ? Ws[jj * dr + k] : 0.f;  // rows d .. dP-1 hold zeros
          else
            w[q] = (kvalid && jj < d) ? Wr[static_cast<int64_t>(jj) * dr + k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kTT; ++u) {
          const int i = slot * kTT + u;
          const f32x4 a = ld4(&Xs[(0 * kTile + i) * kJC + j]);
          const f32x4 p = ld4(&Xs[(1 * kTile + i) * kJC + j]);
          const f32x4 n = ld4(&Xs[(2 * kTile + i) * kJC + j]);
          pa[u] = fmaf(a.x, w[0], pa[u]);
          pa[u] = fmaf(a.y, w[1], pa[u]);
          pa[u] = fmaf(a.z, w[2], pa[u]);
          pa[u] = fmaf(a.w, w[3], pa[u]);
          pp[u] = fmaf(p.x, w[0], pp[u]);
          pp[u] = fmaf(p.y, w[1], pp[u]);
          pp[u] = fmaf(p.z, w[2], pp[u]);
          pp[u] = fmaf(p.w, w[3], pp[u]);
          pn[u] = fmaf(n.x, w[0], pn[u]);
          pn[u] = fmaf(n.y, w[1], pn[u]);
          pn[u] = fmaf(n.z, w[2], pn[u]);
          pn[u] = fmaf(n.w, w[3], pn[u]);
        }
      }
    }
    const float ek = kvalid ? R[static_cast<int64_t>(rel) * ldR + k] : 0.f;
#pragma unroll
    for (int u = 0; u < kTT; ++u) {
      const int i = slot * kTT + u;
      if (kvalid && i < n_here) {
        const int64_t at = static_cast<int64_t>(base + i) * dr + k;
        const int64_t plane = static_cast<int64_t>(B) * dr;
        proj[at] = pa[u];
        proj[plane + at] = pp[u];
        proj[2 * plane + at] = pn[u];
        const float he = pa[u] + ek;
        const float dp = he - pp[u], dn = he - pn[u];
        dpos[u] = fmaf(dp, dp, dpos[u]);
        dneg[u] = fmaf(dn, dn, dneg[u]);
        sq[0] = fmaf(pa[u], pa[u], sq[0]);
        sq[1] = fmaf(ek, ek, sq[1]);
        sq[2] = fmaf(pp[u], pp[u], sq[2]);
        sq[3] = fmaf(pn[u], pn[u], sq[3]);
      }
    }
  }
  float ls = 0.f;
#pragma unroll
  for (int u = 0; u < kTT; ++u) {
    const float x = group_sum<kKC>(dpos[u]) - group_sum<kKC>(dneg[u]);
    const int i = slot * kTT + u;
    if (i < n_here) {
      // −logsigmoid(neg − pos) = softplus(x) and σ(x), both from exp(−|x|) <= 1
      const float ex = expf(-fabsf(x));
      ls += fmaxf(x, 0.f) + log1pf(ex);
      if (lane == 0) coef[base + i] = (x >= 0.f ? 1.f : ex) / (1.f + ex) / fB;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) sq[q] = group_sum<kKC>(sq[q]);
  if (lane == 0) {
    red[slot][0] = ls;
#pragma unroll
    for (int q = 0; q < 4; ++q) red[slot][1 + q] = sq[q];
  }
  __syncthreads();
  if (threadIdx.x < kPart) {
    float s = 0.f;
    if (threadIdx.x < 5) {
      s = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kSlots; ++w) s += red[w][threadIdx.x];
    }
    part[static_cast<int64_t>(blockIdx.x) * kPart + threadIdx.x] = s;
  }
}

// The second stage: the tiles' partials in tile order per thread, then a fixed tree.
//   norms = (‖A‖, ‖E_r‖, ‖P‖, ‖N‖);  loss = Σ softplus / B + (Σ norms · reg) / batch_size_kg
__global__ __launch_bounds__(kBlock) void k_kgl_finish(const float* __restrict__ part,
                                                       int n_tiles, float fB, float reg,
                                                       float bs, float* __restrict__ norms,
                                                       float* __restrict__ loss) {
  __shared__ float sh[5][kBlock];
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t = threadIdx.x; t < n_tiles; t += kBlock) {
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] += part[static_cast<int64_t>(t) * kPart + q];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) sh[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int m = kBlock / 2; m >= 1; m >>= 1) {
    if (static_cast<int>(threadIdx.x) < m) {
#pragma unroll
      for (int q = 0; q < 5; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + m];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float total = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float nq = sqrtf(sh[1 + q][0]);
      norms[q] = nq;
      total += nq;
    }
    loss[0] = sh[0][0] / fB + total * reg / bs;
  }
}

// ---- backward -------------------------------------------------------------------------------
// With u = a + e − p, w = a + e − n, c_i = σ(pos_i − neg_i)/B (saved) and λ = reg/batch_size_kg:
//   g_a = grad·(2c(n − p) + λ a/‖A‖)   g_p = grad·(−2c u + λ p/‖P‖)   g_n = grad·(2c w + λ n/‖N‖)
//   g_e = grad·(2c(n − p) + λ e/‖E_r‖);  a norm that is exactly 0 contributes 0 (as torch.norm).
struct Coefs {
  float g, cA, cE, cP, cN;
};

__device__ __forceinline__ Coefs load_coefs(const float* __restrict__ norms,
                                            const float* __restrict__ grad, float reg, float bs) {
  const float lam = reg / bs;
  Coefs c;
  c.g = grad[0];
  c.cA = norms[0] > 0.f ? lam / norms[0] : 0.f;
  c.cE = norms[1] > 0.f ? lam / norms[1] : 0.f;
  c.cP = norms[2] > 0.f ? lam / norms[2] : 0.f;
  c.cN = norms[3] > 0.f ? lam / norms[3] : 0.f;
  return c;
}

// Gs[s][i][0 .. kGC) = (g_a, g_p, g_n) of the tile's triple i, columns [kc, kc + kGC); zeros
// past column dr and past the tile's end
__device__ __forceinline__ void grad_chunk(float* __restrict__ Gs, const float* __restrict__ proj,
                                           const float* __restrict__ coef,
                                           const float* __restrict__ Rr, int B, int dr, int base,
                                           int n_here, int kc, const Coefs& cf) {
  const int64_t plane = static_cast<int64_t>(B) * dr;
  for (int e = threadIdx.x; e < kTile * kGC; e += kBlock) {
    const int i = e / kGC, kk = e - i * kGC;
    const int k = kc + kk;
    float ga = 0.f, gp = 0.f, gn = 0.f;
    if (i < n_here && k < dr) {
      const int64_t at = static_cast<int64_t>(base + i) * dr + k;
      const float a = proj[at], p = proj[plane + at], n = proj[2 * plane + at];
      const float c2 = 2.f * coef[base + i];
      const float he = a + Rr[k];
      ga = cf.g * fmaf(c2, n - p, cf.cA * a);
      gp = cf.g * fmaf(-c2, he - p, cf.cP * p);
      gn = cf.g * fmaf(c2, he - n, cf.cN * n);
    }
    Gs[(0 * kTile + i) * kGC + kk] = ga;
    Gs[(1 * kTile + i) * kGC + kk] = gp;
    Gs[(2 * kTile + i) * kGC + kk] = gn;
  }
}

// (a) the row gradients dX_s,i = W_r · g_s,i, written as G[s·B + triple][d]. Thread (slot, lane):
// embedding column j = 32·pass + lane of the slot's kTT triples; W_r stands in LDS with an odd
// row stride (lanes walk its rows) or is read through the cache.
template <bool W_LDS>
__global__ __launch_bounds__(kBlock) void k_kgl_bwd_rows(
    const float* __restrict__ W, const float* __restrict__ R, int64_t ldR, int n_rel, int d,
    int dr, const int32_t* __restrict__ grp_perm, const int64_t* __restrict__ rel_off, int B,
    float reg, float bs, const float* __restrict__ proj, const float* __restrict__ coef,
    const float* __restrict__ norms, const float* __restrict__ grad, float* __restrict__ G) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int sh_id[kTile];
  float* Gs = smem;
  float* Ws = smem + 3 * kTile * kGC;

  const uint8_t* const all_relations = nullptr;
  HGD_KG_FIND_TILE(n_rel, rel_off, all_relations, rel, base, end);
  if (rel < 0) return;
  const int n_here = min(kTile, end - base);
  tile_rows(Rows{}, grp_perm, base, n_here, nullptr, sh_id);
  const float* Wr = W + static_cast<int64_t>(rel) * d * dr;
  const float* Rr = R + static_cast<int64_t>(rel) * ldR;
  const int drP = dr | 1;
  if constexpr (W_LDS) {
    for (int idx = threadIdx.x; idx < d * dr; idx += kBlock) {
      const int j = idx / dr, k = idx - j * dr;
      Ws[j * drP + k] = Wr[idx];
    }
  }
  const Coefs cf = load_coefs(norms, grad, reg, bs);
  const int lane = threadIdx.x & (kKC - 1);
  const int slot = threadIdx.x / kKC;
  const int n_kc = (dr + kGC - 1) / kGC;

  for (int j0 = 0; j0 < d; j0 += kKC) {
    const int j = j0 + lane;
    const bool jvalid = j < d;
    float acc[3][kTT];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int u = 0; u < kTT; ++u) acc[s][u] = 0.f;
    for (int kc = 0; kc < dr; kc += kGC) {
      __syncthreads();  // the ids and W_r are written; the previous chunk is read
      if (n_kc > 1 || j0 == 0) grad_chunk(Gs, proj, coef, Rr, B, dr, base, n_here, kc, cf);
      __syncthreads();
      const int knP = (min(kGC, dr - kc) + 3) & ~3;
      for (int kk = 0; kk < knP; kk += 4) {
        float w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = kc + kk + q;
          if constexpr (W_LDS)
            w[q] = (jvalid && k < dr) ? Ws[j * drP + k] : 0.f;
          else
            w[q] = (jvalid && k < dr) ? Wr[static_cast<int64_t>(j) * dr + k] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
          for (int u = 0; u < kTT; ++u) {
            const f32x4 g = ld4(&Gs[(s * kTile + slot * kTT + u) * kGC + kk]);
            acc[s][u] = fmaf(g.x, w[0], acc[s][u]);
            acc[s][u] = fmaf(g.y, w[1], acc[s][u]);
            acc[s][u] = fmaf(g.z, w[2], acc[s][u]);
            acc[s][u] = fmaf(g.w, w[3], acc[s][u]);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
#pragma unroll
      for (int u = 0; u < kTT; ++u) {
        const int i = slot * kTT + u;
        if (jvalid && i < n_here)
          G[(static_cast<int64_t>(s) * B + sh_id[i]) * d + j] = acc[s][u];
      }
    }
  }
}

// (b) + (c) a tile's share of dW_r and dR_r: out[tile] = [d·dr | dr] floats,
//   out[j·dr + k] = Σ_i (x_h,i[j]·g_a,i[k] + x_p,i[j]·g_p,i[k] + x_n,i[j]·g_n,i[k]),
//   out[d·dr + k] = Σ_i g_e,i[k], i over the tile's triples in grouped order. Thread (slot, lane)
//   owns the 2 × 2 × 4 outputs j = jc + 32·jj + 4·slot + q, k = kc + 32·kk + lane of a 64 × 64
//   chunk pair.
__global__ __launch_bounds__(kBlock) void k_kgl_bwd_params(
    Rows rows, const float* __restrict__ R, int64_t ldR, int n_rel, int d, int dr,
    const int32_t* __restrict__ grp_perm, const int64_t* __restrict__ rel_off, int B, float reg,
    float bs, const float* __restrict__ proj, const float* __restrict__ coef,
    const float* __restrict__ norms, const float* __restrict__ grad, float* __restrict__ Wp) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int sh_row[3][kTile];
  float* Gs = smem;
  float* Xs = smem + 3 * kTile * kGC;

  const uint8_t* const all_relations = nullptr;
  HGD_KG_FIND_TILE(n_rel, rel_off, all_relations, rel, base, end);
  if (rel < 0) return;
  const int n_here = min(kTile, end - base);
  tile_rows(rows, grp_perm, base, n_here, sh_row, nullptr);
  const float* Rr = R + static_cast<int64_t>(rel) * ldR;
  const Coefs cf = load_coefs(norms, grad, reg, bs);
  const int per = d * dr + dr;
  float* out = Wp + static_cast<int64_t>(blockIdx.x) * per;
  const int lane = threadIdx.x & (kKC - 1);
  const int slot = threadIdx.x / kKC;
  const int64_t plane = static_cast<int64_t>(B) * dr;

  for (int kc = 0; kc < dr; kc += kGC) {
    __syncthreads();  // the rows' numbers are written; the previous chunk is read
    grad_chunk(Gs, proj, coef, Rr, B, dr, base, n_here, kc, cf);
    if (threadIdx.x < kGC && kc + static_cast<int>(threadIdx.x) < dr) {
      const int k = kc + threadIdx.x;
      const float le = cf.cE * Rr[k];
      float s = 0.f;
      for (int i = 0; i < n_here; ++i) {
        const int64_t at = static_cast<int64_t>(base + i) * dr + k;
        s += cf.g * fmaf(2.f * coef[base + i], proj[2 * plane + at] - proj[plane + at], le);
      }
      out[d * dr + k] = s;
    }
    for (int jc = 0; jc < d; jc += kJC) {
      __syncthreads();  // the gradients are written; the previous rows are read
      stage_rows(rows, sh_row, n_here, jc, d, kJC, Xs);
      __syncthreads();
      float acc[2][2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[a][b][q] = 0.f;
      for (int i = 0; i < n_here; ++i) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const float g0 = Gs[(s * kTile + i) * kGC + lane];
          const float g1 = Gs[(s * kTile + i) * kGC + kKC + lane];
          const f32x4 x0 = ld4(&Xs[(s * kTile + i) * kJC + slot * 4]);
          const f32x4 x1 = ld4(&Xs[(s * kTile + i) * kJC + kKC + slot * 4]);
          const float xs[2][4] = {{x0.x, x0.y, x0.z, x0.w}, {x1.x, x1.y, x1.z, x1.w}};
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              acc[a][0][q] = fmaf(xs[a][q], g0, acc[a][0][q]);
              acc[a][1][q] = fmaf(xs[a][q], g1, acc[a][1][q]);
            }
        }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = jc + a * kKC + slot * 4 + q;
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int k = kc + b * kKC + lane;
            if (j < d && k < dr) out[j * dr + k] = acc[a][b][q];
          }
        }
    }
  }
}

// dW[r] | dR[r] = the partials of r's tiles added in tile order, one element per thread; a
// relation without triples gets exact zeros.
__global__ __launch_bounds__(kBlock) void k_kgl_combine(const float* __restrict__ Wp,
                                                        const int64_t* __restrict__ rel_off,
                                                        int d, int dr, float* __restrict__ dW,
                                                        float* __restrict__ dR) {
  const int r = blockIdx.y;
  const int first = kg_tiles_before(r, rel_off);
  const int cnt = static_cast<int>(rel_off[r + 1] - rel_off[r]);
  const int nt = (cnt + kTile - 1) / kTile;
  const int per = d * dr + dr;
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= per) return;
  const float* p = Wp + static_cast<int64_t>(first) * per + e;
  float s = 0.f;
  for (int t = 0; t < nt; ++t) s += p[static_cast<int64_t>(t) * per];
  if (e < d * dr)
    dW[static_cast<int64_t>(r) * d * dr + e] = s;
  else
    dR[static_cast<int64_t>(r) * dr + (e - d * dr)] = s;
}

int64_t n_tiles(int64_t B, int32_t n_rel) {
  return (B + kTile - 1) / kTile + (n_rel < B ? n_rel : B);
}

size_t part_bytes(int64_t B, int32_t n_rel) {
  return align_up(static_cast<size_t>(n_tiles(B, n_rel)) * kPart * sizeof(float));
}

hgd_status check_common(const char* fn, const float* const* x, const int64_t* ld, const float* W,
                        const float* R, int64_t ldR, int32_t n_rel, int32_t d, int32_t dr,
                        const int32_t* grp_perm, const int64_t* rel_off, int64_t B,
                        int64_t batch_size_kg) {
  HGD_REQUIRE(d > 0 && dr > 0, "%s: d and dr must be > 0 (got %d, %d)", fn, d, dr);
  HGD_REQUIRE(static_cast<int64_t>(d) * dr <= (1 << 24), "%s: d * dr out of range", fn);
  HGD_REQUIRE(B > 0, "%s: B must be > 0 (the mean over no triples is undefined)", fn);
  HGD_REQUIRE(B < 0x7fffffffLL / 3, "%s: B out of range", fn);
  HGD_REQUIRE(n_rel > 0 && n_rel <= 65535, "%s: n_rel must be in [1, 65535] (got %d)", fn,
              n_rel);
  HGD_REQUIRE(batch_size_kg > 0, "%s: batch_size_kg must be > 0", fn);
  HGD_REQUIRE(ld[0] >= d && ld[1] >= d && ld[2] >= d && ldR >= dr,
              "%s: the rows' leading dimensions must be >= d and ldR >= dr", fn);
  HGD_REQUIRE(x[0] && x[1] && x[2] && W && R && grp_perm && rel_off, "%s: null pointer", fn);
  return HGD_OK;
}

}  // namespace
}  // namespace hgd

using namespace hgd;

extern "C" size_t hgd_kg_loss_workspace_size(int64_t B, int32_t n_rel, int32_t d, int32_t dr) {
  if (B <= 0 || n_rel <= 0 || d <= 0 || dr <= 0) return 0;
  const size_t per = (static_cast<size_t>(d) + 1) * dr;
  return part_bytes(B, n_rel) +
         align_up(static_cast<size_t>(n_tiles(B, n_rel)) * per * sizeof(float));
}

extern "C" hgd_status hgd_kg_loss_forward(
    const float* xh, int64_t ldh, const int32_t* ih, const float* xp, int64_t ldp,
    const int32_t* ip, const float* xn, int64_t ldn, const int32_t* in, const float* W,
    const float* R, int64_t ldR, int32_t n_rel, int32_t d, int32_t dr, const int32_t* grp_perm,
    const int64_t* rel_off, int64_t B, float reg_kg, int64_t batch_size_kg, float* proj,
    float* coef, float* norms, float* loss, void* workspace, size_t workspace_bytes,
    void* stream) {
  clear_error();
  const char* fn = "hgd_kg_loss_forward";
  const float* x[3] = {xh, xp, xn};
  const int64_t ld[3] = {ldh, ldp, ldn};
  if (hgd_status st = check_common(fn, x, ld, W, R, ldR, n_rel, d, dr, grp_perm, rel_off, B,
                                   batch_size_kg))
    return st;
  HGD_REQUIRE(proj && coef && norms && loss, "%s: null pointer", fn);
  const size_t need = part_bytes(B, n_rel);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", fn,
                workspace == nullptr ? size_t{0} : workspace_bytes, need);
  const Rows rows{{xh, xp, xn}, {ldh, ldp, ldn}, {ih, ip, in}};
  const int tiles = static_cast<int>(n_tiles(B, n_rel));
  const size_t w_bytes = static_cast<size_t>((d + 3) & ~3) * dr * sizeof(float);
  const bool w_lds = w_bytes <= kWLdsMax;
  const size_t lds = 3 * kTile * kJC * sizeof(float) + (w_lds ? w_bytes : 0);
  float* part = static_cast<float*>(workspace);
  const int iB = static_cast<int>(B);
  if (w_lds)
    hipLaunchKernelGGL(k_kgl_forward<true>, dim3(tiles), dim3(kBlock), lds, as_stream(stream),
                       rows, W, R, ldR, n_rel, d, dr, grp_perm, rel_off, iB, proj, coef, part);
  else
    hipLaunchKernelGGL(k_kgl_forward<false>, dim3(tiles), dim3(kBlock), lds, as_stream(stream),
                       rows, W, R, ldR, n_rel, d, dr, grp_perm, rel_off, iB, proj, coef, part);
  if (hgd_status st = check_launch(fn)) return st;
  hipLaunchKernelGGL(k_kgl_finish, dim3(1), dim3(kBlock), 0, as_stream(stream), part, tiles,
                     static_cast<float>(B), reg_kg, static_cast<float>(batch_size_kg), norms,
                     loss);
  return check_launch(fn);
}

extern "C" hgd_status hgd_kg_loss_backward(
    const float* xh, int64_t ldh, const int32_t* ih, const float* xp, int64_t ldp,
    const int32_t* ip, const float* xn, int64_t ldn, const int32_t* in, const float* W,
    const float* R, int64_t ldR, int32_t n_rel, int32_t d, int32_t dr, const int32_t* grp_perm,
    const int64_t* rel_off, int64_t B, float reg_kg, int64_t batch_size_kg, const float* proj,
    const float* coef, const float* norms, const float* grad, float* G, float* dW, float* dR,
    void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  const char* fn = "hgd_kg_loss_backward";
  const float* x[3] = {xh, xp, xn};
  const int64_t ld[3] = {ldh, ldp, ldn};
  if (hgd_status st = check_common(fn, x, ld, W, R, ldR, n_rel, d, dr, grp_perm, rel_off, B,
                                   batch_size_kg))
    return st;
  HGD_REQUIRE(proj && coef && norms && grad, "%s: null pointer", fn);
  HGD_REQUIRE((dW == nullptr) == (dR == nullptr), "%s: dW and dR go together", fn);
  const size_t need = dW != nullptr ? hgd_kg_loss_workspace_size(B, n_rel, d, dr) : 0;
  if (need && (workspace == nullptr || workspace_bytes < need))
    return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", fn,
                workspace == nullptr ? size_t{0} : workspace_bytes, need);
  const Rows rows{{xh, xp, xn}, {ldh, ldp, ldn}, {ih, ip, in}};
  const int tiles = static_cast<int>(n_tiles(B, n_rel));
  const int iB = static_cast<int>(B);
  const float bs = static_cast<float>(batch_size_kg);
  if (G != nullptr) {
    const size_t w_bytes = static_cast<size_t>(d) * (dr | 1) * sizeof(float);
    const bool w_lds = w_bytes <= kWLdsMax;
    const size_t lds = 3 * kTile * kGC * sizeof(float) + (w_lds ? w_bytes : 0);
    if (w_lds)
      hipLaunchKernelGGL(k_kgl_bwd_rows<true>, dim3(tiles), dim3(kBlock), lds, as_stream(stream),
                         W, R, ldR, n_rel, d, dr, grp_perm, rel_off, iB, reg_kg, bs, proj, coef,
                         norms, grad, G);
    else
      hipLaunchKernelGGL(k_kgl_bwd_rows<false>, dim3(tiles), dim3(kBlock), lds,
                         as_stream(stream), W, R, ldR, n_rel, d, dr, grp_perm, rel_off, iB,
                         reg_kg, bs, proj, coef, norms, grad, G);
    if (hgd_status st = check_launch(fn)) return st;
  }
  if (dW != nullptr) {
    float* Wp = reinterpret_cast<float*>(static_cast<char*>(workspace) + part_bytes(B, n_rel));
    const size_t lds = 3 * kTile * (kGC + kJC) * sizeof(float);
    hipLaunchKernelGGL(k_kgl_bwd_params, dim3(tiles), dim3(kBlock), lds, as_stream(stream), rows,
                       R, ldR, n_rel, d, dr, grp_perm, rel_off, iB, reg_kg, bs, proj, coef,
                       norms, grad, Wp);
    if (hgd_status st = check_launch(fn)) return st;
    const int per = d * dr + dr;
    hipLaunchKernelGGL(k_kgl_combine, dim3(grid_for(per, kBlock), n_rel), dim3(kBlock), 0,
                       as_stream(stream), Wp, rel_off, d, dr, dW, dR);
    if (hgd_status st = check_launch(fn)) return st;
  }
  return HGD_OK;
}
