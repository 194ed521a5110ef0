// The tile code of the view-attention kernels (view_attention.hip) and of the kernels built on
// them (cf_loss.hip): a workgroup owns kVaRows rows, the views stand in LDS as f32 rows and as
// split-bf16 planes in MFMA-fragment order, and each wave holds one 16-column tile of every
// weight matrix as split fragments in registers. Everything here sits in an anonymous namespace:
// every including translation unit gets its own copies (not part of the ABI).
#pragma once

#include <algorithm>

#include "linear_common.h"

namespace hgd {
namespace {

using namespace lin;

constexpr int kVaRows = 32;  // rows of a workgroup's block (two 16-row MFMA tiles)

// K = d padded to 32·KQ (zeros); NCT padded column tiles, one per wave; RTW row tiles side by
// side (the narrow widths), RI row tiles in turn per wave.
template <int KQ>
struct VA {
  static constexpr int KP = 32 * KQ;
  static constexpr int NCT = 2 * KQ;
  static constexpr int RTW = NCT <= 4 ? 2 : 1;
  static constexpr int RI = 2 / RTW;
  static constexpr int THREADS = 64 * NCT * RTW;
  static constexpr int LPR = KP / 4;   // float4 pieces of a row
  static constexpr int LDF = KP + 4;   // f32 row stride: 16 rows' 16-byte reads on distinct banks
  static constexpr size_t F32_BYTES = static_cast<size_t>(kVaRows) * LDF * 4;
  static constexpr size_t PLANE_BYTES = static_cast<size_t>(2) * KQ * 1024;  // one bf16 term
  static constexpr size_t OPER_BYTES = 3 * PLANE_BYTES;                      // one operand
  static constexpr size_t LDS_FWD = 2 * F32_BYTES + 3 * OPER_BYTES;
  static constexpr size_t LDS_BWD = 4 * F32_BYTES + 3 * OPER_BYTES;
};

// Byte offset of the 16-byte fragment slot (row j of a 16-row tile, k-group g, k step q) inside a
// 1 KB (tile, k step) block: the staged row GEMM's conflict-free swizzle (linear_x3s.hip).
__device__ __forceinline__ int frag_slot(int j, int g, int q) {
  return (g * 16 + (j ^ (2 * g + (q & 1)))) * 16;
}

// The three bf16 terms of the float4 piece c of block row rl → the operand's planes.
template <int KQ>
__device__ __forceinline__ void put_planes(char* oper, int rl, int c, f32x4 x) {
  bf16x4 h, m, l;
  split3x4(x, h, m, l);
  const int q = c >> 3;
  const int off = ((rl >> 4) * KQ + q) * 1024 + frag_slot(rl & 15, c & 3, q) + ((c >> 2) & 1) * 8;
  *reinterpret_cast<bf16x4*>(oper + off) = h;
  *reinterpret_cast<bf16x4*>(oper + VA<KQ>::PLANE_BYTES + off) = m;
  *reinterpret_cast<bf16x4*>(oper + 2 * VA<KQ>::PLANE_BYTES + off) = l;
}

// acc = Σ_k x[row i16 of tile rt][k] · Bm[k][this wave's column]: 6 MFMAs per k step, the
// accumulators ready to be read when it returns (mfma_drain).
template <int KQ>
__device__ __forceinline__ f32x4 tile_product(const char* oper, int rt, int i16, int g,
                                              const bf16x8 (&w)[KQ][3]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const char* at = oper + (rt * KQ + q) * 1024 + frag_slot(i16, g, q);
    const bf16x8 xh = *reinterpret_cast<const bf16x8*>(at);
    const bf16x8 xm = *reinterpret_cast<const bf16x8*>(at + VA<KQ>::PLANE_BYTES);
    const bf16x8 xl = *reinterpret_cast<const bf16x8*>(at + 2 * VA<KQ>::PLANE_BYTES);
    acc = mfma_x3(w[q][0], w[q][1], w[q][2], xh, xm, xl, acc, false);
  }
  mfma_drain();
  __builtin_amdgcn_sched_barrier(0);  // the next product's fragment reads stay behind this one
  return acc;
}

// This lane's split fragments of column `col` of Bm[k][n] = W[k·sk + n·sn], zeros past d.
template <int KQ>
__device__ __forceinline__ void load_wfrag(const float* __restrict__ W, int d, int sk, int sn,
                                           int col, int g, bf16x8 (&w)[KQ][3]) {
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * q + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
      const bool ok = col < d && k < d;  // (a clamped load and a select: no branch per element)
      const float x = W[ok ? k * sk + col * sn : 0];
      v[j] = ok ? x : 0.f;
    }
    split3(v, w[q][0], w[q][1], w[q][2]);
  }
  // one matrix at a time: the loads of the next one are not hoisted over this one's split
  __builtin_amdgcn_sched_barrier(0);
}

// NA row sources of a block: load_block brings this thread's float4 pieces into registers (zeros
// past row n and column d: a clamped load and a select, no branch), store_block writes them to
// the f32 rows in LDS and, for the first two sources (the views), to their bf16 planes.
template <int KQ, int NA>
struct Stage {
  using C = VA<KQ>;
  static constexpr int PER = kVaRows * C::LPR;  // float4 pieces of one source
  static constexpr int F = NA * PER / C::THREADS;
  static_assert(NA * PER % C::THREADS == 0, "the pieces divide among the threads");
};

template <int KQ, int NA>
__device__ __forceinline__ void load_block(const float* const (&src)[NA], const int64_t (&ld)[NA],
                                           int64_t r0, int64_t n, int d,
                                           f32x4 (&v)[Stage<KQ, NA>::F]) {
  using S = Stage<KQ, NA>;
#pragma unroll
  for (int u = 0; u < S::F; ++u) {
    const int f = threadIdx.x + S::C::THREADS * u;
    const int a = f / S::PER, rem = f % S::PER;
    const int rl = rem / S::C::LPR, c = rem % S::C::LPR;
    const bool ok = r0 + rl < n && 4 * c < d;  // (clamped to the first piece, then a select)
    v[u] = ld4(src[a] + (ok ? (r0 + rl) * ld[a] + 4 * c : 0));
    if (!ok) v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

template <int KQ, int NA>
__device__ __forceinline__ void store_block(const f32x4 (&v)[Stage<KQ, NA>::F], char* smem,
                                            char* Zp) {
  using S = Stage<KQ, NA>;
#pragma unroll
  for (int u = 0; u < S::F; ++u) {
    const int f = threadIdx.x + S::C::THREADS * u;
    const int a = f / S::PER, rem = f % S::PER;
    const int rl = rem / S::C::LPR, c = rem % S::C::LPR;
    *reinterpret_cast<f32x4*>(smem + a * S::C::F32_BYTES + (rl * S::C::LDF + 4 * c) * 4) = v[u];
    if (a < 2) put_planes<KQ>(Zp + a * S::C::OPER_BYTES, rl, c, v[u]);
  }
}

__device__ __forceinline__ f32x4 tanh4(f32x4 x) {
  return f32x4{tanhf(x.x), tanhf(x.y), tanhf(x.z), tanhf(x.w)};
}

// σ(q) from one exponential of −|q| <= 0: finite for every finite q
__device__ __forceinline__ float sigmoid_stable(float q) {
  const float e = expf(-fabsf(q));
  return (q >= 0.f ? 1.f : e) / (1.f + e);
}

// dW1 += the second view's product, db1 += its column sums (a fixed two-term sum per element)
__global__ __launch_bounds__(kBlock) void k_va_add(float* __restrict__ dW1,
                                                   const float* __restrict__ T, int nW,
                                                   float* __restrict__ db1,
                                                   const float* __restrict__ Tb, int nb) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e < nW)
    dW1[e] += T[e];
  else if (e < nW + nb)
    db1[e - nW] += Tb[e - nW];
}

// workgroups of a launch: the row blocks, at most one resident round of the current device
// (occupancy × CUs, and the kernel's dynamic-LDS limit, looked up once per device)
constexpr int kMaxDevices = 64;

template <typename K>
hgd_status resident_blocks(K kern, int threads, size_t lds, int (&cached)[kMaxDevices],
                           int* out) {
  int dev = 0;
  HGD_HIP(hipGetDevice(&dev));
  const bool slot = dev >= 0 && dev < kMaxDevices;
  if (slot && cached[dev] != 0) {
    *out = cached[dev];
    return HGD_OK;
  }
  if (lds > 65536)
    HGD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds)));
  int nb = 0, cus = 0;
  HGD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, lds));
  HGD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  *out = std::max(1, nb) * std::max(1, cus);
  if (slot) cached[dev] = *out;
  return HGD_OK;
}

inline bool al16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al16r(const float* p, int64_t ld) { return al16p(p) && ld % 4 == 0; }

}  // namespace
}  // namespace hgd
