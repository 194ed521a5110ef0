// Fused score, mask and top-K: from the two embedding tables and the rated-items CSR straight to
// the [n_rows, k] recommendation lists. No score goes to HBM.
//
// Reference (paths relative to its HD_SELFRec directory): GraphRecommender.test()
// (base/graph_recommender.py:61-92) scores one user (user_emb[u]·item_embᵀ), sets the rated items
// to -10e8 (:79-80) and calls find_k_largest (util/algorithm.py:143-173), whose closed form
// (topk.hip) is the first K of  seed = {(c_j, j) : j < K} ∪ stream = {(c_i, i)}
// by score descending, seed before stream, index ascending.
//
// k_rank_stream — one 256-thread workgroup per (64-user block, item segment):
//   * a wave owns 16 users; their embeddings are f32 MFMA A fragments in registers
//     (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 sums), d padded with zeros to DP;
//   * item rows stream through LDS in tiles of 64 (next tile prefetched into registers while the
//     current one is consumed); every (user, item) score is the same DP/4-long MFMA chain from a
//     zero accumulator, so its bits do not depend on the row, the tile, the segment or the launch;
//   * a score leaves its accumulator only if it beats the user's running threshold τ (the k-th
//     best effective score at the last compaction; NaN = "fewer than k held, take everything").
//     Such a raw score is appended to the user's 128 candidate slots in LDS as (score, id). While
//     τ < mask_value every item is appended (a rated item with a lower raw score is raised to
//     mask_value and may enter the list);
//   * after a tile, a user with more than 64 candidates is compacted by its wave: the new
//     candidates are looked up in the user's rated row (one binary search per lane, side by
//     side) and become mask_value if rated, then the 128 slots are sorted in registers
//     (bitonic, shuffles) by (score desc, id asc), k kept, τ raised. A masked candidate that no
//     longer beats τ simply sorts out. Ids
//     ascend within a segment, so a later score equal to τ can never win its tie: the filter is a
//     strict >. A user gets at most 64 candidates per tile and holds at most 64 before it, so the
//     slots never overflow. Candidate state is touched by the owning wave only;
//   * the effective scores of items 0..k-1 (the seed copies) are stored by segment 0 at its
//     first compaction, which still holds the whole first tile; at the end each (user, segment) writes its k best to the workspace.
// k_rank_merge — one workgroup per row: the k seeds and the segments' candidates, sorted with
// cand_before in rounds of at most 2,048; the first k are the list. A second launch, no flags.
#include "device_util.h"
#include "hgd_internal.h"
#include "topk_common.h"

namespace hgd {
namespace rank {

constexpr int kTU = 64;        // users per workgroup (4 waves × 16 rows)
constexpr int kTI = 64;        // items per tile (>= HGD_RANK_MAX_K: the seeds are in one tile)
constexpr int kSlots = 128;    // candidate slots per user (k kept + one tile's appends)
constexpr int kMaxSeg = 256;   // segments per user block
constexpr int kCUs = 256;      // the constant CU count of the automatic segment choice
constexpr int kMergeCap = 2048;
constexpr int32_t kNoId = 0x7fffffff;

static_assert(kTI >= HGD_RANK_MAX_K, "the seed window must lie in the first tile");
static_assert(kSlots == 128 && kSlots - kTI >= HGD_RANK_MAX_K, "slots: k kept + a tile");

struct Args {
  const float* U;
  int64_t ldu;
  const float* V;
  int64_t ldi;
  int64_t n_items;
  int32_t d;
  const int32_t* users;
  int64_t n_rows;
  const int64_t* rp;
  const int32_t* rc;
  float mask;
  int32_t k;
  int32_t nseg;
  int64_t tiles_per_seg;
  float* ws_seed;   // [n_rows, k]
  float* ws_sc;     // [n_rows, nseg, k]
  int32_t* ws_id;   // [n_rows, nseg, k]
};

template <int DP>
struct Geo {
  static constexpr int C4 = DP / 4;             // float4 pieces of a row
  static constexpr int Q4 = DP / 16;            // float4 fragments per lane
  static constexpr int LDR = DP + 4;            // padded LDS row (floats): 16 rows, 16 bank quads
  static constexpr int PER = kTI * C4 / 256;    // float4s per thread per tile
  static constexpr size_t LDS = sizeof(float) * kTI * LDR + 8u * kTU * kSlots + 12u * kTU;
};

// a before b: score descending, id ascending (±0.0 equal, as cand_before)
__device__ __forceinline__ bool before(float as, int32_t ai, float bs, int32_t bi) {
  return as > bs || (as == bs && ai < bi);
}

// 128 (score, id) pairs of one wave, position p = lane + 64·j in (sj, ij), sorted best first.
__device__ __forceinline__ void sort128(float (&s)[2], int32_t (&id)[2], int lane) {
#pragma unroll
  for (int size = 2; size <= 128; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride == 64) {  // size 128: partner in the same lane, best-first everywhere
        if (before(s[1], id[1], s[0], id[0])) {
          const float ts = s[0];
          const int32_t ti = id[0];
          s[0] = s[1];
          id[0] = id[1];
          s[1] = ts;
          id[1] = ti;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int p = lane + 64 * j;
          const float os = __shfl_xor(s[j], stride, 64);
          const int32_t oi = __shfl_xor(id[j], stride, 64);
          const bool keep_better = ((p & size) == 0) == ((lane & stride) == 0);
          const bool other_better = before(os, oi, s[j], id[j]);
          if (keep_better == other_better) {
            s[j] = os;
            id[j] = oi;
          }
        }
      }
    }
  }
}

// The wave sorts the candidates of user ul (row `row` of the call). Slots from n_eff on still hold
// raw scores: each is looked up in the user's rated row first (one candidate per lane, the
// binary searches run side by side) and becomes mask_value if rated. Segment 0 (seeds == true)
// stores the effective scores of items 0..k-1, all of which are among the candidates of the
// first compaction, as the seed copies. In the stream: keep k, raise τ. At the end: write the k
// best (padded with (-inf, kNoId) when the segment held fewer) to out_sc / out_id when non-null.
__device__ __forceinline__ void compact(const Args& a, float* s_sc, int32_t* s_id, float* s_tau,
                                        int* s_cnt, int* s_eff, int ul, int64_t row, bool seeds,
                                        int lane, float* out_sc, int32_t* out_id) {
  const int k = a.k;
  const int cnt = min(s_cnt[ul], kSlots);
  const int n_eff = s_eff[ul];
  int64_t r_lo = 0, r_end = 0;
  if (a.rp) {
    const int64_t u = a.users ? a.users[row] : row;
    r_lo = a.rp[u];
    r_end = a.rp[u + 1];
  }
  float s[2];
  int32_t id[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = lane + 64 * j;
    s[j] = e < cnt ? s_sc[ul * kSlots + e] : -INFINITY;
    id[j] = e < cnt ? s_id[ul * kSlots + e] : kNoId;
    if (e >= n_eff && e < cnt) {
      int64_t lo = r_lo, hi = r_end;
      while (lo < hi) {  // first rated column >= id; at most 64 halvings of [lo, hi)
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.rc[mid] < id[j])
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < r_end && a.rc[lo] == id[j]) s[j] = a.mask;
    }
    if (seeds && e < cnt && id[j] < k) a.ws_seed[row * k + id[j]] = s[j];
  }
  sort128(s, id, lane);
  if (out_sc) {
    if (lane < k) {
      out_sc[lane] = s[0];
      out_id[lane] = id[0];
    }
    return;
  }
  if (lane < k) {  // k <= 64: the kept entries are the lanes' first elements
    s_sc[ul * kSlots + lane] = s[0];
    s_id[ul * kSlots + lane] = id[0];
  }
  if (cnt >= k && lane == k - 1) s_tau[ul] = s[0];
  if (lane == 0) {
    s_cnt[ul] = min(cnt, k);
    s_eff[ul] = min(cnt, k);
  }
}

// The float4 pieces of tile t a thread stages: rows past the catalogue and columns past d are zero.
template <int DP>
__device__ __forceinline__ void tile_load(const Args& a, int64_t t, bool vec,
                                          f32x4 (&v)[Geo<DP>::PER]) {
  using G = Geo<DP>;
#pragma unroll
  for (int i = 0; i < G::PER; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int64_t item = t * kTI + e / G::C4;
    const int c = 4 * (e % G::C4);
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (item < a.n_items && c < a.d) {
      const float* p = a.V + item * a.ldi + c;
      if (vec && c + 4 <= a.d) {
        x = ld4(p);
      } else {
        x.x = p[0];
        if (c + 1 < a.d) x.y = p[1];
        if (c + 2 < a.d) x.z = p[2];
        if (c + 3 < a.d) x.w = p[3];
      }
    }
    v[i] = x;
  }
}

template <int DP>
__device__ __forceinline__ void tile_store(float* s, const f32x4 (&v)[Geo<DP>::PER]) {
  using G = Geo<DP>;
#pragma unroll
  for (int i = 0; i < G::PER; ++i) {
    const int e = threadIdx.x + 256 * i;
    *reinterpret_cast<f32x4*>(s + (e / G::C4) * G::LDR + 4 * (e % G::C4)) = v[i];
  }
}

// A raw score that passed the filter: appended to user ul's slots (at most kTI per tile and user
// on top of at most kSlots - kTI held, so pos < kSlots; the guard keeps a broken invariant inside
// the slots).
__device__ __forceinline__ void append(float* s_sc, int32_t* s_id, int* s_cnt, int ul,
                                       int32_t item, float raw) {
  const int pos = atomicAdd(&s_cnt[ul], 1);
  if (pos < kSlots) {
    s_sc[ul * kSlots + pos] = raw;
    s_id[ul * kSlots + pos] = item;
  }
}

template <int DP>
__global__ __launch_bounds__(256) void k_rank_stream(Args a) {
  using G = Geo<DP>;
  extern __shared__ __align__(16) unsigned char rank_smem[];
  float* s_stage = reinterpret_cast<float*>(rank_smem);
  float* s_sc = s_stage + kTI * G::LDR;
  int32_t* s_id = reinterpret_cast<int32_t*>(s_sc + kTU * kSlots);
  float* s_tau = reinterpret_cast<float*>(s_id + kTU * kSlots);
  int* s_cnt = reinterpret_cast<int*>(s_tau + kTU);
  int* s_eff = s_cnt + kTU;  // slots [0, s_eff) hold effective scores already

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int seg = blockIdx.y;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kTU + 16 * wave;
  const int64_t n_tiles = (a.n_items + kTI - 1) / kTI;
  const int64_t t_first = seg * a.tiles_per_seg;
  const int64_t t_begin = t_first < n_tiles ? t_first : n_tiles;
  const int64_t t_end = t_begin + a.tiles_per_seg < n_tiles ? t_begin + a.tiles_per_seg : n_tiles;
  const bool vec = (reinterpret_cast<uintptr_t>(a.V) & 15) == 0 && a.ldi % 4 == 0;

  if (threadIdx.x < kTU) {
    s_tau[threadIdx.x] = __builtin_nanf("");
    s_cnt[threadIdx.x] = 0;
    s_eff[threadIdx.x] = 0;
  }

  // A fragments: lane l holds U[row0 + (l & 15)][4(l >> 4) + 16q + c] (rows past the end: the
  // last row's, never listed)
  float af[G::Q4][4];
  {
    const int64_t r = row0 + (lane & 15) < a.n_rows ? row0 + (lane & 15) : a.n_rows - 1;
    const int64_t u = a.users ? a.users[r] : r;
    const float* up = a.U + u * a.ldu;
#pragma unroll
    for (int q = 0; q < G::Q4; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int kk = 4 * (lane >> 4) + 16 * q + c;
        af[q][c] = kk < a.d ? up[kk] : 0.f;
      }
  }
  // the four rows whose scores this lane receives (C rows 4(l >> 4) + r)
  bool rv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rv[r] = row0 + 4 * (lane >> 4) + r < a.n_rows;

  f32x4 v[G::PER];
  if (t_begin < t_end) {
    tile_load<DP>(a, t_begin, vec, v);
    tile_store<DP>(s_stage, v);
  }
  __syncthreads();
  for (int64_t t = t_begin; t < t_end; ++t) {
    const bool more = t + 1 < t_end;
    if (more) tile_load<DP>(a, t + 1, vec, v);
    float tau[4];
    bool all[4];  // every item is a candidate: the seeds' tile, or τ below mask_value (a rated
                  // item with a lower raw score is raised to it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      tau[r] = s_tau[16 * wave + 4 * (lane >> 4) + r];
      all[r] = t == 0 || (a.rp != nullptr && !(a.mask <= tau[r]));
    }
    // the four 16-item sub-tiles' chains side by side (independent accumulators keep the MFMA
    // pipe busy behind the LDS reads); each chain is still q-major, c-minor from zero
    constexpr int kST = kTI / 16;
    const float* brow = s_stage + (lane & 15) * G::LDR + 4 * (lane >> 4);
    f32x4 s[kST];
#pragma unroll
    for (int st = 0; st < kST; ++st) s[st] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < G::Q4; ++q) {
      f32x4 b[kST];
#pragma unroll
      for (int st = 0; st < kST; ++st)
        b[st] = *reinterpret_cast<const f32x4*>(brow + 16 * st * G::LDR + 16 * q);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int st = 0; st < kST; ++st) s[st] = mfma4(af[q][c], b[st][c], s[st]);
    }
    // the accumulators are read under branches below: the MFMA → VALU wait states placed here
    // (hipcc places them only when the first read shares the chain's basic block)
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
    for (int st = 0; st < kST; ++st) {
      // s[st][r] = <U[users[row0 + 4(l >> 4) + r]], V[item]>
      const int64_t item = t * kTI + 16 * st + (lane & 15);
      const bool iok = item < a.n_items;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (iok && rv[r] && (all[r] || !(s[st][r] <= tau[r])))
          append(s_sc, s_id, s_cnt, 16 * wave + 4 * (lane >> 4) + r, static_cast<int32_t>(item),
                 s[st][r]);
      }
    }
    __syncthreads();  // the tile is consumed; the wave's appends are visible to the wave
    {
      const bool need = lane < 16 && s_cnt[16 * wave + (lane & 15)] > kSlots - kTI;
      unsigned long long m = __ballot(need);
      while (m) {  // at most 16 users
        const int ul = 16 * wave + __builtin_ctzll(m);
        m &= m - 1;
        compact(a, s_sc, s_id, s_tau, s_cnt, s_eff, ul, row0 - 16 * wave + ul, seg == 0, lane,
                nullptr, nullptr);
      }
    }
    if (more) tile_store<DP>(s_stage, v);
    __syncthreads();
  }
  // the k best of every (user, segment), in (score desc, id asc) order
  for (int j = 0; j < 16; ++j) {
    const int64_t R = row0 + j;
    if (R >= a.n_rows) break;  // uniform over the wave
    const int64_t o = (R * a.nseg + seg) * a.k;
    compact(a, s_sc, s_id, s_tau, s_cnt, s_eff, 16 * wave + j, R, seg == 0, lane, a.ws_sc + o,
            a.ws_id + o);
  }
}

__global__ __launch_bounds__(kTopkBlock) void k_rank_merge(const float* __restrict__ ws_seed,
                                                           const float* __restrict__ ws_sc,
                                                           const int32_t* __restrict__ ws_id,
                                                           int nseg, int k,
                                                           int32_t* __restrict__ out_ids,
                                                           float* __restrict__ out_scores) {
  __shared__ Cand s_c[kMergeCap];
  const int64_t r = blockIdx.x;
  const int64_t base = r * nseg * k;
  const int total = nseg * k;
  for (int t = threadIdx.x; t < k; t += kTopkBlock) s_c[t] = Cand{ws_seed[r * k + t], t, 1};
  for (int pos = 0; pos < total;) {  // each round takes at least kMergeCap - k candidates
    const int take = min(total - pos, kMergeCap - k);
    for (int t = threadIdx.x; t < take; t += kTopkBlock)
      s_c[k + t] = Cand{ws_sc[base + pos + t], ws_id[base + pos + t], 0};
    int n2 = 1;
    while (n2 < k + take) n2 <<= 1;
    for (int t = k + take + threadIdx.x; t < n2; t += kTopkBlock)
      s_c[t] = Cand{-INFINITY, kNoId, 0};
    __syncthreads();
    bitonic_sort(s_c, n2);
    pos += take;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < k; t += kTopkBlock) {
    out_ids[r * k + t] = s_c[t].i;
    out_scores[r * k + t] = s_c[t].s;
  }
}

// Segments per user block: the caller's count, or by shape (enough workgroups for two per CU of a
// 256-CU part, at least 8 tiles each), never more than tiles or kMaxSeg.
inline int segments_for(int64_t n_rows, int64_t n_items, int32_t n_segments) {
  const int64_t tiles = (n_items + kTI - 1) / kTI;
  const int64_t blocks = (n_rows + kTU - 1) / kTU;
  int64_t n = n_segments;
  if (n == 0) {
    n = (2 * kCUs + blocks - 1) / std::max<int64_t>(1, blocks);
    n = std::min(n, tiles / 8);
  }
  n = std::min(n, std::min<int64_t>(tiles, kMaxSeg));
  return static_cast<int>(std::max<int64_t>(1, n));
}

// (row, segment) candidate lists the workspace holds. Explicit segments: the lists launched. By
// shape: a bound of them that does not shrink when an argument grows (rows·segments <=
// 64·(2·kCUs + blocks), and <= rows·min(tiles, kMaxSeg)).
inline int64_t workspace_lists(int64_t n_rows, int64_t n_items, int32_t n_segments) {
  if (n_segments != 0) return n_rows * segments_for(n_rows, n_items, n_segments);
  const int64_t tiles = (n_items + kTI - 1) / kTI;
  const int64_t blocks = (n_rows + kTU - 1) / kTU;
  return std::min<int64_t>(kTU * (2 * kCUs + blocks),
                           n_rows * std::max<int64_t>(1, std::min<int64_t>(tiles, kMaxSeg)));
}

template <int DP>
hgd_status launch(const Args& a, dim3 grid, hipStream_t st) {
  const void* kern = reinterpret_cast<const void*>(&k_rank_stream<DP>);
  static bool lds_set = false;
  if (!lds_set) {
    if (Geo<DP>::LDS > 65536)
      HGD_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(Geo<DP>::LDS)));
    lds_set = true;
  }
  hipLaunchKernelGGL(k_rank_stream<DP>, grid, dim3(256), Geo<DP>::LDS, st, a);
  return check_launch("hgd_rank_topk");
}

}  // namespace rank
}  // namespace hgd

using namespace hgd;

extern "C" void hgd_rank_topk_geometry(int32_t* users_per_block, int32_t* items_per_tile,
                                       int32_t* candidate_slots) {
  if (users_per_block) *users_per_block = rank::kTU;
  if (items_per_tile) *items_per_tile = rank::kTI;
  if (candidate_slots) *candidate_slots = rank::kSlots;
}

extern "C" size_t hgd_rank_topk_workspace_size(int64_t n_rows, int64_t n_items, int32_t k,
                                               int32_t n_segments) {
  if (n_rows <= 0 || n_items <= 0 || k <= 0 || n_segments < 0) return 0;
  const size_t kk = static_cast<size_t>(k);
  return align_up(sizeof(float) * static_cast<size_t>(n_rows) * kk) +
         8u * static_cast<size_t>(rank::workspace_lists(n_rows, n_items, n_segments)) * kk;
}

extern "C" hgd_status hgd_rank_topk(const float* user_emb, int64_t ldu, const float* item_emb,
                                    int64_t ldi, int64_t n_items, int32_t d,
                                    const int32_t* users, int64_t n_rows,
                                    const int64_t* rated_rowptr, const int32_t* rated_cols,
                                    float mask_value, int32_t k, int32_t n_segments,
                                    int32_t* out_ids, float* out_scores, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  clear_error();
  HGD_REQUIRE(n_rows >= 0 && n_items >= 0 && n_items < 0x80000000LL, "hgd_rank_topk: sizes");
  HGD_REQUIRE(d >= 1 && ldu >= d && ldi >= d, "hgd_rank_topk: d = %d, ldu = %lld, ldi = %lld", d,
              (long long)ldu, (long long)ldi);
  HGD_REQUIRE(k >= 1 && k <= n_items, "hgd_rank_topk: k = %d of %lld items", k,
              (long long)n_items);
  HGD_REQUIRE(n_segments >= 0, "hgd_rank_topk: n_segments = %d", n_segments);
  if (k > HGD_RANK_MAX_K)
    return fail(HGD_ERR_UNSUPPORTED, "hgd_rank_topk: k = %d > HGD_RANK_MAX_K = %d", k,
                HGD_RANK_MAX_K);
  if (d > HGD_RANK_MAX_D)
    return fail(HGD_ERR_UNSUPPORTED, "hgd_rank_topk: d = %d > HGD_RANK_MAX_D = %d", d,
                HGD_RANK_MAX_D);
  if (n_rows == 0) return HGD_OK;
  HGD_REQUIRE(user_emb && item_emb && out_ids && out_scores, "hgd_rank_topk: null pointer");
  HGD_REQUIRE(((reinterpret_cast<uintptr_t>(user_emb) | reinterpret_cast<uintptr_t>(item_emb)) &
               3) == 0, "hgd_rank_topk: tables must be 4-byte aligned");
  const int64_t blocks = (n_rows + rank::kTU - 1) / rank::kTU;
  if (n_rows > 0x7fffffffLL) return fail(HGD_ERR_UNSUPPORTED, "hgd_rank_topk: too many rows");
  const size_t need = hgd_rank_topk_workspace_size(n_rows, n_items, k, n_segments);
  if (!workspace || workspace_bytes < need)
    return fail(HGD_ERR_WORKSPACE, "hgd_rank_topk: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  HGD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
              "hgd_rank_topk: workspace must be 4-byte aligned");

  rank::Args a;
  a.U = user_emb;
  a.ldu = ldu;
  a.V = item_emb;
  a.ldi = ldi;
  a.n_items = n_items;
  a.d = d;
  a.users = users;
  a.n_rows = n_rows;
  a.rp = rated_rowptr;
  a.rc = rated_cols;
  a.mask = mask_value;
  a.k = k;
  a.nseg = rank::segments_for(n_rows, n_items, n_segments);
  const int64_t tiles = (n_items + rank::kTI - 1) / rank::kTI;
  a.tiles_per_seg = (tiles + a.nseg - 1) / a.nseg;
  char* w = static_cast<char*>(workspace);
  a.ws_seed = reinterpret_cast<float*>(w);
  w += align_up(sizeof(float) * static_cast<size_t>(n_rows) * k);
  const size_t lists = static_cast<size_t>(n_rows) * a.nseg * k;
  a.ws_sc = reinterpret_cast<float*>(w);
  a.ws_id = reinterpret_cast<int32_t*>(w + sizeof(float) * lists);

  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(a.nseg));
  hipStream_t st = as_stream(stream);
  hgd_status rc;
  if (d <= 64)
    rc = rank::launch<64>(a, grid, st);
  else if (d <= 128)
    rc = rank::launch<128>(a, grid, st);
  else
    rc = rank::launch<256>(a, grid, st);
  if (rc != HGD_OK) return rc;
  hipLaunchKernelGGL(rank::k_rank_merge, dim3(static_cast<unsigned>(n_rows)), dim3(kTopkBlock),
                     0, st, a.ws_seed, a.ws_sc, a.ws_id, a.nseg, k, out_ids, out_scores);
  return check_launch("hgd_rank_topk");
}
