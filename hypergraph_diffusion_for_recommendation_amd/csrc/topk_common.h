// The candidate record and ordering of find_k_largest's closed form, shared by
// the row top-K (topk.hip) and the fused score / mask / top-K (rank.hip). Not part of the ABI.
#pragma once

#include "hgd_internal.h"

namespace hgd {

constexpr int kTopkBlock = 256;

struct Cand {
  float s;
  int32_t i;
  int32_t seed;  // 1 = seed copy (precedes stream entries of equal score)
};

// a before b in the output order
__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
  if (a.s != b.s) return a.s > b.s;
  if (a.seed != b.seed) return a.seed > b.seed;
  return a.i < b.i;
}

// In-LDS bitonic sort of n (a power of two) candidates by a kTopkBlock-thread workgroup, best
// first.
__device__ __forceinline__ void bitonic_sort(Cand* c, int n) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < n / 2; t += kTopkBlock) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool asc = (lo & size) == 0;  // "ascending" = best first in this sub-sequence
        const bool swap = asc ? cand_before(c[hi], c[lo]) : cand_before(c[lo], c[hi]);
        if (swap) {
          const Cand tmp = c[lo];
          c[lo] = c[hi];
          c[hi] = tmp;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace hgd
