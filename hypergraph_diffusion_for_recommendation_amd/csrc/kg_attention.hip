// KHGRec's knowledge-graph attention on the device (include/hgd.h, "KG attention"):
//   hgd_kg_attention_scores   Equation 4 for a whole batch of triples, one launch for all relations
//   hgd_kg_attention_softmax  Equation 5, torch.sparse.softmax(dim=1) over the uncoalesced batch
// Both are fp32 with every sum in a fixed order and no atomics: two runs are bitwise equal, and a
// triple's score does not depend on where in the batch it stands.
#include <cmath>

#include "device_util.h"
#include "hgd_internal.h"
#include "kg_tile.h"

namespace hgd {
namespace {

// ---- scores ---------------------------------------------------------------------------------
// A workgroup owns kTile consecutive triples of ONE relation in the relation-grouped order and
// reads that relation's W_r once: into LDS when it fits (kWLdsMax), through the cache otherwise.
// The two gathered embedding rows of every triple are staged in LDS kJC columns at a time.
// Thread (slot, lane): relation-space column k = 32·kc + lane of the kTT triples of its slot;
// the projections are fmaf chains over the embedding columns in ascending order, the sum over k
// a per-lane chain over kc followed by a 32-lane xor butterfly.
constexpr int kTile = kKgTile;
constexpr int kKC = 32;
constexpr int kJC = 128;
constexpr int kSlots = kBlock / kKC;
constexpr int kTT = kTile / kSlots;
constexpr int kStage = 8;  // staged elements per thread and row kind whose loads overlap
constexpr size_t kWLdsMax = 30 * 1024;  // + 32 KB of staged rows + the ids: inside 64 KB

static_assert(kSlots * kTT == kTile && kKC == 32 && kJC % 4 == 0, "tile geometry");

template <bool W_LDS>
__global__ __launch_bounds__(kBlock) void k_kg_scores(
    const float* __restrict__ E, int64_t ldE, const float* __restrict__ W,
    const float* __restrict__ R, int64_t ldR, int n_rel, int d, int dr,
    const int32_t* __restrict__ h, const int32_t* __restrict__ t,
    const int32_t* __restrict__ grp_perm, const int64_t* __restrict__ rel_off,
    const uint8_t* __restrict__ rel_enable, float* __restrict__ v) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int sh_h[kTile], sh_t[kTile], sh_id[kTile];
  float* Eh = smem;
  float* Et = smem + kTile * kJC;
  float* Ws = smem + 2 * kTile * kJC;

  // which (relation, tile) this workgroup is (kg_tile.h)
  HGD_KG_FIND_TILE(n_rel, rel_off, rel_enable, rel, base, end);
  if (rel < 0) return;  // a surplus workgroup (the grid is the bound ⌈B/kTile⌉ + relations)
  const int n_here = min(kTile, end - base);

  if (threadIdx.x < kTile) {
    const int i = threadIdx.x;
    int id = 0, hh = 0, tt = 0;
    if (i < n_here) {
      id = grp_perm[base + i];
      hh = h[id];
      tt = t[id];
    }
    sh_id[i] = id;
    sh_h[i] = hh;  // (a tile's unused slots project entity 0 and store nothing)
    sh_t[i] = tt;
  }
  const float* Wr = W + static_cast<int64_t>(rel) * d * dr;
  const int dP = (d + 3) & ~3;
  if constexpr (W_LDS) {
    for (int idx = threadIdx.x; idx < dP * dr; idx += kBlock)
      Ws[idx] = idx < d * dr ? Wr[idx] : 0.f;
  }

  const int lane = threadIdx.x & (kKC - 1);
  const int slot = threadIdx.x / kKC;
  const int n_jc = (d + kJC - 1) / kJC;
  float part[kTT];
#pragma unroll
  for (int u = 0; u < kTT; ++u) part[u] = 0.f;

  for (int k0 = 0; k0 < dr; k0 += kKC) {
    const int k = k0 + lane;
    const bool kvalid = k < dr;
    float ph[kTT], pt[kTT];
#pragma unroll
    for (int u = 0; u < kTT; ++u) ph[u] = pt[u] = 0.f;
    for (int jc = 0; jc < n_jc; ++jc) {
      const int j0 = jc * kJC;
      const int jn = min(kJC, d - j0);
      const int jnP = (jn + 3) & ~3;
      __syncthreads();  // the ids and W_r are written; the previous chunk's rows are read
      if (n_jc > 1 || k0 == 0) {
        // kStage elements of both rows per thread in flight before the first LDS store, so the
        // gathers' round trips overlap
        const int total = kTile * jnP;
        for (int e0 = threadIdx.x; e0 < total; e0 += kBlock * kStage) {
          float a[kStage], b[kStage];
#pragma unroll
          for (int u = 0; u < kStage; ++u) {
            const int e = e0 + u * kBlock;
            a[u] = b[u] = 0.f;
            if (e < total) {
              const int i = e / jnP, j = e - i * jnP;
              if (j < jn) {
                a[u] = E[static_cast<int64_t>(sh_h[i]) * ldE + j0 + j];
                b[u] = E[static_cast<int64_t>(sh_t[i]) * ldE + j0 + j];
              }
            }
          }
#pragma unroll
          for (int u = 0; u < kStage; ++u) {
            const int e = e0 + u * kBlock;
            if (e < total) {
              const int i = e / jnP, j = e - i * jnP;
              Eh[i * kJC + j] = a[u];
              Et[i * kJC + j] = b[u];
            }
          }
        }
      }
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
          const f32x4 a = ld4(&Eh[(slot * kTT + u) * kJC + j]);
          const f32x4 b = ld4(&Et[(slot * kTT + u) * kJC + j]);
          ph[u] = fmaf(a.x, w[0], ph[u]);
          ph[u] = fmaf(a.y, w[1], ph[u]);
          ph[u] = fmaf(a.z, w[2], ph[u]);
          ph[u] = fmaf(a.w, w[3], ph[u]);
          pt[u] = fmaf(b.x, w[0], pt[u]);
          pt[u] = fmaf(b.y, w[1], pt[u]);
          pt[u] = fmaf(b.z, w[2], pt[u]);
          pt[u] = fmaf(b.w, w[3], pt[u]);
        }
      }
    }
    const float rk = kvalid ? R[static_cast<int64_t>(rel) * ldR + k] : 0.f;
#pragma unroll
    for (int u = 0; u < kTT; ++u)
      if (kvalid) part[u] = fmaf(pt[u], tanhf(ph[u] + rk), part[u]);
  }
#pragma unroll
  for (int u = 0; u < kTT; ++u) {
    const float s = group_sum<kKC>(part[u]);
    const int i = slot * kTT + u;
    if (lane == 0 && i < n_here) v[sh_id[i]] = s;
  }
}

// ---- softmax --------------------------------------------------------------------------------
// A workgroup owns kBlock consecutive head rows, one per thread (most rows of a sampled batch are
// empty or a few entries long, and a wave per row would spend its time starting waves):
//   1. a row of up to kShortRow entries is done by its own lane, sequentially;
//   2. a row of up to kLongRow entries by its wave, one such row after the other;
//   3. a longer row (it may be the whole batch) by the whole workgroup.
// A run of equal (row, column) is summed in order by the one worker that owns its first entry: a
// row that is a single run is summed by a single lane in every form (the in-order sum is the rule).
// Worker `id` of `NT` (1, 64 or kBlock) owns the entries b + id, b + id + NT, … in all passes, so
// it only ever re-reads what it wrote itself.
constexpr int kShortRow = 8;
constexpr int kLongRow = 512;
constexpr int kWaves = kBlock / 64;

template <bool MAX>
__device__ __forceinline__ float wave_reduce(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float o = __shfl_xor(x, m, 64);
    x = MAX ? fmaxf(x, o) : x + o;
  }
  return x;
}

template <int NT, bool MAX>
__device__ __forceinline__ float row_reduce(float x, float* red) {
  if constexpr (NT == 1) return x;
  x = wave_reduce<MAX>(x);
  if constexpr (NT == kBlock) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) x = MAX ? fmaxf(x, red[w]) : x + red[w];
    __syncthreads();
  }
  return x;
}

template <int NT>
__device__ __forceinline__ void softmax_row(int64_t b, int64_t e, const int32_t* __restrict__ col,
                                            const int32_t* __restrict__ perm,
                                            const float* __restrict__ v, float* __restrict__ s,
                                            float* __restrict__ val, float* red) {
  const int id = NT == 1 ? 0 : (NT == 64 ? (threadIdx.x & 63) : threadIdx.x);
  // 1. the sum of every duplicate group, in order, by the owner of its first member
  float m = -INFINITY;
  for (int64_t p = b + id; p < e; p += NT) {
    const int c = col[p];
    if (p == b || col[p - 1] != c) {
      float a = v[perm[p]];
      for (int64_t q = p + 1; q < e && col[q] == c; ++q) a += v[perm[q]];
      s[p] = a;
      m = fmaxf(m, a);
    }
  }
  m = row_reduce<NT, true>(m, red);  // 2. the row max
  float z = 0.f;                     // 3. exponentiate and sum
  for (int64_t p = b + id; p < e; p += NT) {
    if (p == b || col[p - 1] != col[p]) {
      const float ex = expf(s[p] - m);
      s[p] = ex;
      z += ex;
    }
  }
  z = row_reduce<NT, false>(z, red);
  for (int64_t p = b + id; p < e; p += NT)  // 4. normalise; the other members carry exactly 0
    val[p] = (p == b || col[p - 1] != col[p]) ? s[p] / z : 0.f;
}

__global__ __launch_bounds__(kBlock) void k_kg_softmax(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ perm, int64_t n_rows, int64_t B, const float* __restrict__ v,
    float* __restrict__ s, float* __restrict__ val) {
  __shared__ float red[kWaves];
  __shared__ unsigned long long long_rows[kWaves];
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kBlock;
  const int64_t row = row0 + threadIdx.x;
  int b = 0, e = 0;  // (B < 2^31)
  if (row < n_rows) {
    b = static_cast<int>(rowptr[row]);
    e = static_cast<int>(rowptr[row + 1]);
  }
  const int len = e - b;
  if (len > 0 && len <= kShortRow) softmax_row<1>(b, e, col, perm, v, s, val, red);
  unsigned long long todo = __ballot(len > kShortRow && len <= kLongRow);
  while (todo) {  // (wave-uniform: every lane walks the same rows)
    const int L = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1;
    softmax_row<64>(__shfl(b, L, 64), __shfl(e, L, 64), col, perm, v, s, val, red);
  }
  const unsigned long long lng = __ballot(len > kLongRow);
  if ((threadIdx.x & 63) == 0) long_rows[threadIdx.x >> 6] = lng;
  __syncthreads();
  for (int w = 0; w < kWaves; ++w) {  // (workgroup-uniform: the masks come from LDS)
    unsigned long long m = long_rows[w];
    while (m) {
      const int L = __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      const int64_t r = row0 + w * 64 + L;
      softmax_row<kBlock>(rowptr[r], rowptr[r + 1], col, perm, v, s, val, red);
    }
  }
  // the entries past the last row (the triples of disabled relations) carry 0
  const int64_t live = rowptr[n_rows];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t p = live + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; p < B;
       p += stride)
    val[p] = 0.f;
}

}  // namespace
}  // namespace hgd

using namespace hgd;

extern "C" hgd_status hgd_kg_attention_scores(
    const float* E, int64_t ldE, int64_t n_ent, const float* W, const float* R, int64_t ldR,
    int32_t n_rel, int32_t d, int32_t dr, const int32_t* h, const int32_t* t,
    const int32_t* grp_perm, const int64_t* rel_off, const uint8_t* rel_enable, int64_t B,
    float* v, void* stream) {
  clear_error();
  HGD_REQUIRE(d > 0 && dr > 0, "hgd_kg_attention_scores: d and dr must be > 0 (got %d, %d)", d,
              dr);
  HGD_REQUIRE(B >= 0 && n_ent >= 0 && n_rel >= 0, "hgd_kg_attention_scores: negative sizes");
  HGD_REQUIRE(ldE >= d && ldR >= dr,
              "hgd_kg_attention_scores: ldE must be >= d and ldR >= dr");
  if (B == 0) return HGD_OK;
  HGD_REQUIRE(B < 0x7fffffffLL, "hgd_kg_attention_scores: B out of range");
  HGD_REQUIRE(E && W && R && h && t && grp_perm && rel_off && v,
              "hgd_kg_attention_scores: null pointer");
  HGD_REQUIRE(n_ent > 0 && n_rel > 0,
              "hgd_kg_attention_scores: triples without entities or relations");
  const int64_t tiles = (B + kTile - 1) / kTile + (n_rel < B ? n_rel : B);
  const size_t w_bytes = static_cast<size_t>((d + 3) & ~3) * dr * sizeof(float);
  const bool w_lds = w_bytes <= kWLdsMax;
  const size_t lds = 2 * kTile * kJC * sizeof(float) + (w_lds ? w_bytes : 0);
  if (w_lds)
    hipLaunchKernelGGL(k_kg_scores<true>, dim3(static_cast<unsigned>(tiles)), dim3(kBlock), lds,
                       as_stream(stream), E, ldE, W, R, ldR, n_rel, d, dr, h, t, grp_perm,
                       rel_off, rel_enable, v);
  else
    hipLaunchKernelGGL(k_kg_scores<false>, dim3(static_cast<unsigned>(tiles)), dim3(kBlock), lds,
                       as_stream(stream), E, ldE, W, R, ldR, n_rel, d, dr, h, t, grp_perm,
                       rel_off, rel_enable, v);
  return check_launch("hgd_kg_attention_scores");
}

extern "C" size_t hgd_kg_attention_softmax_workspace_size(int64_t B) {
  return B > 0 ? align_up(static_cast<size_t>(B) * sizeof(float)) : 0;
}

extern "C" hgd_status hgd_kg_attention_softmax(const int64_t* rowptr, const int32_t* col,
                                               const int32_t* perm, int64_t n_rows, int64_t B,
                                               const float* v, float* val, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  clear_error();
  HGD_REQUIRE(n_rows >= 0 && B >= 0, "hgd_kg_attention_softmax: negative sizes");
  if (B == 0) return HGD_OK;
  HGD_REQUIRE(B < 0x7fffffffLL, "hgd_kg_attention_softmax: B out of range");
  HGD_REQUIRE(rowptr && col && perm && v && val, "hgd_kg_attention_softmax: null pointer");
  HGD_REQUIRE(n_rows > 0, "hgd_kg_attention_softmax: entries without rows");
  const size_t need = hgd_kg_attention_softmax_workspace_size(B);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(HGD_ERR_WORKSPACE, "hgd_kg_attention_softmax: workspace %zu < required %zu",
                workspace == nullptr ? size_t{0} : workspace_bytes, need);
  hipLaunchKernelGGL(k_kg_softmax, dim3(grid_for(n_rows, kBlock)), dim3(kBlock), 0,
                     as_stream(stream), rowptr, col, perm, n_rows, B, v,
                     static_cast<float*>(workspace), val);
  return check_launch("hgd_kg_attention_softmax");
}
