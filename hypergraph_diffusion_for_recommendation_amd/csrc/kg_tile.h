// The (relation, tile) lookup shared by the KG kernels (kg_attention.hip, kg_loss.hip): a
// workgroup owns kKgTile consecutive triples of ONE relation in the relation-grouped order
// (grp_perm / rel_off of include/hgd.h, "KG attention").
#pragma once

#include "device_util.h"

namespace hgd {

constexpr int kKgTile = 32;

// Which (relation, tile) this workgroup (blockIdx.x) is: the tiles of the enabled relations are
// numbered in relation order; every wave finds the answer for itself with a 64-wide prefix scan.
// DECLARES the ints rel, base, end (so: once per function): the tile is the grouped positions
// [base, min(base + kKgTile, end)) of relation rel, end the end of the relation's range;
// rel < 0 for a surplus workgroup (the grid is the bound ⌈B/kKgTile⌉ + relations).
// rel_enable: uint8 [n_rel] or a null pointer.
// A macro, not an inline function: as a function (by reference or returning a struct) the
// compiler lowers the null test of rel_enable differently and k_kg_scores<true>'s code changes;
// expanded in place the device code of kg_attention.hip is what it was before the lookup moved
// here (profiles/kg_loss/device_code_equal.txt).
#define HGD_KG_FIND_TILE(n_rel, rel_off, rel_enable, rel, base, end)               \
  const int lane64_ = threadIdx.x & 63;                                            \
  int rem_ = static_cast<int>(blockIdx.x);                                         \
  int rel = -1, base = 0, end = 0;                                                 \
  do {                                                                             \
    for (int c_ = 0; c_ < (n_rel); c_ += 64) {                                     \
      const int r_ = c_ + lane64_;                                                 \
      int lo_ = 0, cnt_ = 0;                                                       \
      if (r_ < (n_rel) && ((rel_enable) == nullptr || (rel_enable)[r_])) {         \
        lo_ = static_cast<int>((rel_off)[r_]);                                     \
        cnt_ = static_cast<int>((rel_off)[r_ + 1]) - lo_;                          \
      }                                                                            \
      const int nt_ = (cnt_ + ::hgd::kKgTile - 1) / ::hgd::kKgTile;                \
      int inc_ = nt_;                                                              \
      _Pragma("unroll") for (int m_ = 1; m_ < 64; m_ <<= 1) {                      \
        const int o_ = __shfl_up(inc_, m_, 64);                                    \
        if (lane64_ >= m_) inc_ += o_;                                             \
      }                                                                            \
      const int total_ = __shfl(inc_, 63, 64);                                     \
      if (rem_ < total_) {                                                         \
        const unsigned long long hit_ = __ballot(inc_ > rem_);                     \
        const int L_ = __ffsll(static_cast<long long>(hit_)) - 1;                  \
        const int before_ = __shfl(inc_ - nt_, L_, 64);                            \
        const int lo_l_ = __shfl(lo_, L_, 64);                                     \
        const int cnt_l_ = __shfl(cnt_, L_, 64);                                   \
        rel = c_ + L_;                                                             \
        base = lo_l_ + (rem_ - before_) * ::hgd::kKgTile;                          \
        end = lo_l_ + cnt_l_;                                                      \
        break;                                                                     \
      }                                                                            \
      rem_ -= total_;                                                              \
    }                                                                              \
  } while (0)

// The number of tiles of the relations before `rel` (all enabled): the tile id of rel's first
// tile. Every wave computes it for itself (integer sums, so the order is immaterial).
__device__ __forceinline__ int kg_tiles_before(int rel, const int64_t* __restrict__ rel_off) {
  const int lane64 = threadIdx.x & 63;
  int s = 0;
  for (int r = lane64; r < rel; r += 64) {
    const int cnt = static_cast<int>(rel_off[r + 1] - rel_off[r]);
    s += (cnt + kKgTile - 1) / kKgTile;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

}  // namespace hgd
