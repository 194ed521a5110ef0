// Device side of the CSR row-gather SpMM hop (launched by spmm_launch.h): the argument block, the
// gather walks and the kernels, templated on the element types of the gathered table (TX) and
// of the output (TY). Not part of the ABI.
#pragma once

#include "device_util.h"
#include "hgd_internal.h"

namespace hgd {

// TX: element type of the gathered table X, TY: of the output Y (float or bf16; the weights, the
// row scales, the sums and the split plan's partials are fp32 whatever they are)
template <class TX = float, class TY = float>
struct SpmmArgsT {
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  const float* row_scale;
  int64_t row_begin, row_end;
  const TX* X;
  int64_t ldx;
  TY* Y;
  int64_t ldy;
  int32_t d;
  int32_t col0;  // first column handled by this launch (column passes for wide/odd d)
  int32_t epi;
  float slope;
  // split plan
  int64_t heavy_threshold;
  int64_t n_chunks;
  int64_t n_heavy;
  int32_t chunk;
  int32_t seg;  // 1: segmented short-row kernel (plan flag HGD_PLAN_SEGMENTED)
  const int32_t* chunk_heavy;
  const int32_t* heavy_rows;
  const int64_t* heavy_cptr;
  float* partial;  // [n_chunks, d]
  int64_t heavy_blocks;
  hgd_row_epilogue ex;  // used by the EX (hgd_spmm_fused) instantiations only
  // masked hop (hgd_spmm_masked, the MASK instantiations): the edge-dropped matrix of
  // SpAdjDropEdge as a view of its parent — edge e counts iff mask[e] != 0, with weight
  // val[e] / keep (IEEE, as the dropped COO's values)
  const uint8_t* mask;
  float keep;
  // 1 / keep when keep is a power of two (HCCF's 0.5), else 0: then w·inv_keep is w / keep bit
  // for bit (one exact real value, rounded once either way) at one multiply instead of the
  // IEEE division's ~10-instruction sequence per kept entry
  float inv_keep;
  int32_t mask_pair;  // two-batch masked walk (HGD_TUNE_MASK_PAIR)
  // XCD-interleaved column passes (HGD_TUNE_SPMM_PASS_INTERLEAVE): all n_pass column passes of a
  // wide row in ONE launch, the passes of a row block on consecutive workgroups of the same XCD
  int32_t n_pass;     // > 1: interleaved; else the launch covers the one pass at col0
  int32_t pass_cols;  // columns per pass when interleaved
  // source-blocked hop (hgd_spmm_blocked): a launch per source block k over the block-major
  // copy (hgd_spmm_col_blocks), whose rows of block k are a CSR of their own (rowptr =
  // blk_start + k·n_rows); with blk_accum the row adds s·Σ to the Y row the blocks before wrote
  int32_t blk_accum;
  // ordered hop (hgd_spmm_ordered): the rows are walked in the order of hgd_spmm_row_order —
  // position r indexes rowptr / row_scale (the ordered copies) and the row is written to Y row
  // out_row[r]; NULL: Y row r
  const int32_t* out_row;
  // source-blocked hop into a 16-bit Y (hgd_spmm_blocked_dt; read by the 16-bit-TY instantiations
  // only): the running partial of a row lives in fp32 at blk_part + row·ld_part, not in Y — block
  // 0 writes it, the blocks between add to it, and the last block (blk_last) adds it, applies the
  // activation and stores Y once, so Y is rounded once. NULL: Y is written directly
  float* blk_part;
  int64_t ld_part;
  int32_t blk_last;
  // fused row epilogue over a 16-bit table (hgd_spmm_fused_dt; read by the EX instantiations with
  // a 16-bit TX only): a bf16 copy [n_rows, ld_y16] of the row just written to the fp32 Y, rounded
  // from the same registers, for the next layer's hop to gather. NULL: no copy
  bf16* y16;
  int64_t ld_y16;
  // packed entries (hgd_spmm_blocked_packed, the PK instantiations only): col holds one word per
  // nonzero, (column − the block's first source row) | code << idx_bits, X points at the block's
  // first source row and the weight is dict[code] (n_dict floats, copied to LDS per workgroup)
  const float* dict;
  int32_t n_dict;
  int32_t idx_bits;
};
using SpmmArgs = SpmmArgsT<>;

// vals[mask] / keepRate (HCCF.py:224)
template <class TX, class TY>
__device__ __forceinline__ float scale_kept(const SpmmArgsT<TX, TY>& a, float w) {
  return a.inv_keep != 0.f ? w * a.inv_keep : __fdiv_rn(w, a.keep);
}

__device__ __forceinline__ float epilogue(float y, int epi, float slope) {
  if (epi == HGD_EPI_LEAKY_RELU) return y > 0.f ? y : y * slope;
  if (epi == HGD_EPI_RELU) return y > 0.f ? y : 0.f;
  return y;
}

// Cache-policy bits of the tuned variants (hgd_set_tuning(HGD_TUNE_SPMM_POLICY, bits)):
constexpr int kPolNtStore = 1;   // Y rows: non-temporal stores (written once, never re-read here)
constexpr int kPolNtIndex = 2;   // col / val streams: non-temporal loads (read exactly once)
constexpr int kPolNtGather = 4;  // gathered X rows: non-temporal loads
constexpr int kPolPrefetch = 8;  // software-pipelined index batches (see gather_sum)

// Scale, epilogue and store of one finished row r (all G lanes of the group call it together);
// yr is its row of Y (r, or the ordered hop's out_row[r]): everything that belongs to the Y row —
// Y, the epilogue's side arrays (act_out, stats, res1, res2, sum_res, sum_out) and y16 — is
// indexed by yr; r is the position, which the caller read rowptr / row_scale / mask at.
// With EX the hgd_row_epilogue runs in registers: the group holds the whole row (single column
// pass, checked on the host), so the LayerNorm statistics are two group_sum butterflies; over a
// 16-bit table (hgd_spmm_fused_dt) the fp32 row that goes to Y is also stored rounded to a.y16.
// BLK_PART: the caller can be a launch of a source-blocked hop into a 16-bit Y (the row kernel
// without a mask only: the others are the code they were).
template <int G, int VEC, bool EX, bool NT_STORE, class TX = float, class TY = float,
          bool BLK_PART = false>
__device__ __forceinline__ void finish_row(const SpmmArgsT<TX, TY>& a, int64_t r, int64_t yr,
                                           float s, int l, int64_t coff, bool col_ok,
                                           float (&acc)[VEC]) {
  // a 16-bit Y of a source-blocked hop keeps its running partial in the fp32 scratch (blk_part)
  constexpr bool PART = BLK_PART && !EX && sizeof(TY) == 2;
  if constexpr (!EX) {
    if (a.blk_accum) {  // a later block of a column-blocked hop: Y = epi(s·Σ_block + Y)
      float prev[VEC];
      if (col_ok) {
        if constexpr (PART)
          load_vec<VEC>(a.blk_part + yr * a.ld_part + coff, prev);
        else
          load_vec<VEC>(a.Y + yr * a.ldy + coff, prev);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) prev[i] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = epilogue(acc[i] * s + prev[i], a.epi, a.slope);
      if constexpr (PART) {
        if (!a.blk_last) {  // (the activation is HGD_EPI_NONE before the last block)
          if (col_ok) store_vec<VEC>(a.blk_part + yr * a.ld_part + coff, acc);
          return;
        }
      }
      if (col_ok) store_vec<VEC, NT_STORE>(a.Y + yr * a.ldy + coff, acc);
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = epilogue(acc[i] * s, a.epi, a.slope);
  if constexpr (PART) {
    if (a.blk_part && !a.blk_last) {  // block 0 of several: the partial starts in the scratch
      if (col_ok) store_vec<VEC>(a.blk_part + yr * a.ld_part + coff, acc);
      return;
    }
  }
  if constexpr (EX) {
    const hgd_row_epilogue& e = a.ex;
    if (e.act_out && col_ok) store_vec<VEC>(e.act_out + yr * e.ld_act + coff, acc);
    if (e.layer_norm) {
      float t = 0.f;
      if (col_ok) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) t += acc[i];
      }
      const float mu = group_sum<G>(t) / static_cast<float>(a.d);
      t = 0.f;
      if (col_ok) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) t += (acc[i] - mu) * (acc[i] - mu);
      }
      const float rstd = 1.f / sqrtf(group_sum<G>(t) / static_cast<float>(a.d) + e.ln_eps);
      if (e.stats && l == 0) {
        e.stats[2 * yr] = mu;
        e.stats[2 * yr + 1] = rstd;
      }
      if (col_ok) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float gm = e.ln_gamma ? e.ln_gamma[coff + i] : 1.f;
          const float bt = e.ln_beta ? e.ln_beta[coff + i] : 0.f;
          acc[i] = fmaf((acc[i] - mu) * rstd, gm, bt);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] *= e.out_scale;
    if (e.res1 && col_ok) {
      float rv[VEC];
      load_vec<VEC>(e.res1 + yr * e.ld_res1 + coff, rv);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(e.res1_scale, rv[i], acc[i]);
    }
    if (e.res2 && col_ok) {
      float rv[VEC];
      load_vec<VEC>(e.res2 + yr * e.ld_res2 + coff, rv);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(e.res2_scale, rv[i], acc[i]);
    }
  }
  if (col_ok) store_vec<VEC, NT_STORE>(a.Y + yr * a.ldy + coff, acc);
  if constexpr (EX && sizeof(TX) == 2) {
    if (a.y16 && col_ok) store_vec<VEC>(a.y16 + yr * a.ld_y16 + coff, acc);
  }
  if constexpr (EX) {
    const hgd_row_epilogue& e = a.ex;
    if (e.sum_out && col_ok) {
      float rv[VEC];
      load_vec<VEC>(e.sum_res + yr * e.ld_sum_res + coff, rv);
#pragma unroll
      for (int i = 0; i < VEC; ++i) rv[i] = acc[i] + rv[i];
      store_vec<VEC>(e.sum_out + yr * e.ld_sum_out + coff, rv);
    }
  }
}

// Lane l's share of a batch of G column indices (and weights) starting at nonzero eb; with MASK
// also its keep flag (0 past the batch).
template <bool HAS_VAL, int POL, bool MASK = false, class TX = float, class TY = float>
__device__ __forceinline__ void load_index(const SpmmArgsT<TX, TY>& a, int64_t eb, int n, int l,
                                           int& c, float& w, int& keep) {
  c = 0;
  w = 1.f;
  keep = 0;
  if (l < n) {
    if constexpr (MASK) keep = a.mask[eb + l];
    if constexpr (POL & kPolNtIndex) {
      c = __builtin_nontemporal_load(a.col + eb + l);
      if constexpr (HAS_VAL) w = __builtin_nontemporal_load(a.val + eb + l);
    } else {
      c = a.col[eb + l];
      if constexpr (HAS_VAL) w = a.val[eb + l];
    }
  }
}

// Position of the j-th set bit (0-based) of a G-bit group mask: a popcount binary search.
template <int G>
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int j) {
  int pos = 0;
#pragma unroll
  for (int w = G / 2; w >= 1; w >>= 1) {
    const int c = __popcll(m & ((1ull << w) - 1ull));
    if (j >= c) {
      j -= c;
      m >>= w;
      pos += w;
    }
  }
  return pos;
}

// MASK: packs the kept entries of a fetched batch to the front of the group (in edge order) with
// their weights val/keep; returns how many there are. Every lane of the group calls it.
template <int G, bool HAS_VAL, class TX = float, class TY = float>
__device__ __forceinline__ int compact_kept(const SpmmArgsT<TX, TY>& a, int l, int keep, int& c,
                                            float& w) {
  const unsigned long long bal = __ballot(keep != 0);
  const int base = (static_cast<int>(threadIdx.x) & 63) & ~(G - 1);
  const unsigned long long gm =
      G == 64 ? bal : (bal >> base) & ((1ull << (G == 64 ? 0 : G)) - 1ull);
  const int src = nth_set_bit<G>(gm, l);
  if constexpr (HAS_VAL) w = scale_kept(a, w);
  c = __shfl(c, src, G);
  if constexpr (HAS_VAL) w = __shfl(w, src, G);
  return __popcll(gm);
}

// The masked hop's walk (MASK): TWO index batches of G edges per step (2G edges, about G kept
// at keep = 0.5), their kept entries packed in edge order into 2G slots — slot j < G in lane j's
// register a, slot j >= G in lane j-G's register b — so a step gathers as many rows as an
// unmasked batch instead of half as many; the next pair of index batches is loaded before the
// gathers are issued. Sums in edge order: bitwise the one-batch walk and the compacted matrix's.
// PUSH (HGD_TUNE_MASK_PAIR = 2, the default): the packing is ONE forward permute per value and
// batch — each lane sends its entry to its slot (its rank among the kept entries of its batch,
// from a popcount of the lower lanes' keep bits; the dropped entries fill the slots after the
// kept ones, so every batch is a permutation of the group's lanes and no two lanes collide) —
// instead of every lane pulling its slot's entry after a binary search for the j-th set bit
// (nth_set_bit, three per step: ~4 dependent popcount rounds each). Same slots, same sums.
template <int G, int VEC, int U, bool HAS_VAL, int POL, bool PUSH, class TX = float,
          class TY = float>
__device__ __forceinline__ void gather_sum_mask2(const SpmmArgsT<TX, TY>& a, int64_t e0, int64_t e1,
                                                 int l, bool col_ok, float (&acc)[VEC],
                                                 int32_t col0) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  const int64_t coff = static_cast<int64_t>(col0) + static_cast<int64_t>(l) * VEC;
  const int base = (static_cast<int>(threadIdx.x) & 63) & ~(G - 1);
  auto group_bits = [&](int keep) {
    const unsigned long long bal = __ballot(keep != 0);
    return G == 64 ? bal : (bal >> base) & ((1ull << (G == 64 ? 0 : G)) - 1ull);
  };
  auto load2 = [&](int64_t eb, int& c1, float& w1, int& k1, int& c2, float& w2, int& k2) {
    load_index<HAS_VAL, POL, true>(a, eb, static_cast<int>(min(static_cast<int64_t>(G), e1 - eb)),
                                   l, c1, w1, k1);
    const int64_t eb2 = eb + G;
    if (eb2 < e1) {
      load_index<HAS_VAL, POL, true>(
          a, eb2, static_cast<int>(min(static_cast<int64_t>(G), e1 - eb2)), l, c2, w2, k2);
    } else {
      c2 = 0;
      w2 = 1.f;
      k2 = 0;
    }
  };
  int nc1 = 0, nk1 = 0, nc2 = 0, nk2 = 0;
  float nw1 = 1.f, nw2 = 1.f;
  if (e0 < e1) load2(e0, nc1, nw1, nk1, nc2, nw2, nk2);
  for (int64_t eb = e0; eb < e1; eb += 2 * G) {
    const int c1 = nc1, k1 = nk1, c2 = nc2, k2 = nk2;
    const float w1 = nw1, w2 = nw2;
    if (eb + 2 * G < e1) load2(eb + 2 * G, nc1, nw1, nk1, nc2, nw2, nk2);
    const unsigned long long gm1 = group_bits(k1), gm2 = group_bits(k2);
    const int n1 = __popcll(gm1), n2 = __popcll(gm2), n = n1 + n2;
    if (n == 0) continue;  // group-uniform
    // slot l (register a) and slot l + G (register b) of the packed pair
    int ca, cb;
    float wa = 1.f, wb = 1.f;
    if constexpr (PUSH) {
      const unsigned long long below = (1ull << l) - 1ull;  // the group's lanes below l
      const int r1 = __popcll(gm1 & below), r2 = __popcll(gm2 & below);
      // batch 1 → slots [0, G) of register a; batch 2 → slot n1 + rank, i.e. register a of lane
      // (n1 + rank) for slots < G and register b of lane (n1 + rank − G) beyond: one permute
      // modulo G serves both, and each lane's a / b pick (l < n1) is the pull form's
      const int d1 = k1 ? r1 : n1 + (l - r1);
      const int d2 = ((k2 ? r2 : n2 + (l - r2)) + n1) & (G - 1);
      const int a1 = 4 * (base + d1), a2 = 4 * (base + d2);
      const int x1 = __builtin_amdgcn_ds_permute(a1, c1);
      const int x2 = __builtin_amdgcn_ds_permute(a2, c2);
      ca = l < n1 ? x1 : x2;
      cb = x2;
      if constexpr (HAS_VAL) {
        // vals[mask] / keepRate (HCCF.py:224), divided before the move (same IEEE quotient)
        const float v1 = scale_kept(a, w1), v2 = scale_kept(a, w2);
        const float y1 = __int_as_float(__builtin_amdgcn_ds_permute(a1, __float_as_int(v1)));
        const float y2 = __int_as_float(__builtin_amdgcn_ds_permute(a2, __float_as_int(v2)));
        wa = l < n1 ? y1 : y2;
        wb = y2;
      }
    } else {
      const int s1 = nth_set_bit<G>(gm1, l);
      const int s2a = nth_set_bit<G>(gm2, l >= n1 ? l - n1 : 0);
      const int s2b = nth_set_bit<G>(gm2, l + G - n1 < G ? l + G - n1 : 0);
      const int ca1 = __shfl(c1, s1, G), ca2 = __shfl(c2, s2a, G);
      cb = __shfl(c2, s2b, G);
      ca = l < n1 ? ca1 : ca2;
      if constexpr (HAS_VAL) {
        const float wa1 = __shfl(w1, s1, G), wa2 = __shfl(w2, s2a, G);
        wa = scale_kept(a, l < n1 ? wa1 : wa2);
        wb = scale_kept(a, __shfl(w2, s2b, G));
      }
    }
    for (int k = 0; k < n; k += U) {
      const bool hi = k >= G;  // group-uniform: U divides G, so a step stays in one register
      float xv[U][VEC];
      float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = k + u;
        const int c = __shfl(hi ? cb : ca, kk & (G - 1), G);
        if constexpr (HAS_VAL) w[u] = __shfl(hi ? wb : wa, kk & (G - 1), G);
        if (kk < n && col_ok) {
          load_vec<VEC, (POL & kPolNtGather) != 0>(a.X + static_cast<int64_t>(c) * a.ldx + coff,
                                                   xv[u]);
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) xv[u][i] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < n) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            if constexpr (HAS_VAL)
              acc[i] = fmaf(w[u], xv[u][i], acc[i]);
            else
              acc[i] += xv[u][i];
          }
        }
      }
    }
  }
}

// Σ_{e in [e0,e1)} val[e] * X[col[e], cols of this lane], in edge order. With kPolPrefetch the
// index batch b+1 is loaded before the gathers of batch b are issued, so the dependent
// index → gather round trip is paid once per row instead of once per batch of G nonzeros.
// With MASK only the kept edges are summed (same order as over the compacted matrix).
// PK (packed entries, HAS_VAL and no MASK): the index batch is one word per nonzero, the gather
// takes its low idx_bits as the column and the weight is looked up in wdict (the dictionary in
// LDS) from the word's code only where the gathered row is consumed, so no weight is held in
// registers while the gathers are in flight.
template <int G, int VEC, int U, bool HAS_VAL, int POL, bool MASK = false, class TX = float,
          class TY = float, bool PK = false>
__device__ __forceinline__ void gather_sum(const SpmmArgsT<TX, TY>& a, int64_t e0, int64_t e1,
                                           int l, bool col_ok, float (&acc)[VEC], int32_t col0,
                                           const float* wdict = nullptr) {
  static_assert(!PK || (HAS_VAL && !MASK), "packed entries: weighted, no mask");
  // (the index loads of a packed batch are the unweighted ones: one word)
  constexpr bool LD_VAL = HAS_VAL && !PK;
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  const int64_t coff = static_cast<int64_t>(col0) + static_cast<int64_t>(l) * VEC;
  constexpr bool PF = (POL & kPolPrefetch) != 0;
  [[maybe_unused]] const int cmask = PK ? static_cast<int>((1u << a.idx_bits) - 1u) : 0;
  int nxc = 0, nxk = 0;
  float nxw = 1.f;
  if constexpr (PF) {
    if (e0 < e1)
      load_index<LD_VAL, POL, MASK>(
          a, e0, static_cast<int>(min(static_cast<int64_t>(G), e1 - e0)), l, nxc, nxw, nxk);
  }
  for (int64_t eb = e0; eb < e1; eb += G) {
    int n = static_cast<int>(min(static_cast<int64_t>(G), e1 - eb));
    int myc, myk;
    float myw;
    if constexpr (PF) {
      myc = nxc;
      myw = nxw;
      myk = nxk;
      const int64_t en = eb + G;
      if (en < e1)
        load_index<LD_VAL, POL, MASK>(
            a, en, static_cast<int>(min(static_cast<int64_t>(G), e1 - en)), l, nxc, nxw, nxk);
    } else {
      load_index<LD_VAL, POL, MASK>(a, eb, n, l, myc, myw, myk);
    }
    if constexpr (MASK) n = compact_kept<G, HAS_VAL>(a, l, myk, myc, myw);
    for (int k = 0; k < n; k += U) {
      float xv[U][VEC];
      float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = k + u;
        int c = (G == 1) ? myc : __shfl(myc, kk, G);
        if constexpr (PK) c &= cmask;
        if constexpr (LD_VAL) w[u] = (G == 1) ? myw : __shfl(myw, kk, G);
        if (kk < n && col_ok) {
          load_vec<VEC, (POL & kPolNtGather) != 0>(a.X + static_cast<int64_t>(c) * a.ldx + coff,
                                                   xv[u]);
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) xv[u][i] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < n) {
          if constexpr (PK) {
            const unsigned e = static_cast<unsigned>((G == 1) ? myc : __shfl(myc, k + u, G));
            w[u] = wdict[e >> a.idx_bits];
          }
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            if constexpr (HAS_VAL)
              acc[i] = fmaf(w[u], xv[u][i], acc[i]);
            else
              acc[i] += xv[u][i];
          }
        }
      }
    }
  }
}


// MASK with G >= 8 lanes (U | G): the two-batch masked walk unless HGD_TUNE_MASK_PAIR is 0.
template <int G, int VEC, int U, bool HAS_VAL, int POL, bool MASK, class TX = float,
          class TY = float>
__device__ __forceinline__ void masked_or_plain_sum(const SpmmArgsT<TX, TY>& a, int64_t e0,
                                                    int64_t e1, int l, bool col_ok,
                                                    float (&acc)[VEC], int32_t col0) {
  if constexpr (MASK && G >= 8 && G % U == 0) {
    if (a.mask_pair == 2) {
      gather_sum_mask2<G, VEC, U, HAS_VAL, POL, true>(a, e0, e1, l, col_ok, acc, col0);
      return;
    }
    if (a.mask_pair) {
      gather_sum_mask2<G, VEC, U, HAS_VAL, POL, false>(a, e0, e1, l, col_ok, acc, col0);
      return;
    }
  }
  gather_sum<G, VEC, U, HAS_VAL, POL, MASK>(a, e0, e1, l, col_ok, acc, col0);
}

// ORD: the ordered hop (a.out_row set), an instantiation of its own so that every other one is
// the code it was; with EX, MASK and 16-bit TX / TY too (the ordered twins of the fused, masked
// and _dt entry points): position r indexes the ordered copies (rowptr, col, val, row_scale and
// mask, whose entries are in the ordered entry order) and finish_row gets the Y row. PK: the ordered hop over packed entries (a.dict set), one more of its own: the
// dictionary goes to LDS once per workgroup, before any lane leaves.
template <int G, int VEC, int U, bool HAS_VAL, int POL, bool EX, bool MASK = false,
          class TX = float, class TY = float, bool ORD = false, bool PK = false>
__global__ __launch_bounds__(kBlock) void spmm_kernel(SpmmArgsT<TX, TY> a) {
  constexpr int GPB = kBlock / G;
  __shared__ float s_dict[PK ? HGD_SPMM_PACKED_MAX_DICT : 1];  // (unused and dropped unless PK)
  if constexpr (PK) {
    for (int i = threadIdx.x; i < a.n_dict; i += kBlock) s_dict[i] = a.dict[i];
    __syncthreads();
  }
  const int g = threadIdx.x / G;
  const int l = threadIdx.x % G;
  int64_t bid = static_cast<int64_t>(blockIdx.x) - a.heavy_blocks;
  int32_t col0 = a.col0;
  if (a.n_pass > 1) {
    // workgroups are dispatched to the 8 XCDs round-robin (blockIdx mod 8): the n_pass passes of
    // row block (k / n_pass)·8 + x run back to back on XCD x, so the later passes find the row
    // pointers and index stream in that XCD's L2 and fetch the other quarters of the same
    // gathered rows while the DRAM pages are open (no split rows here: heavy_blocks is 0)
    const int64_t x = bid & 7, k = bid >> 3;
    col0 = static_cast<int32_t>((k % a.n_pass) * a.pass_cols);
    bid = (k / a.n_pass) * 8 + x;
  }
  const int64_t coff = static_cast<int64_t>(col0) + static_cast<int64_t>(l) * VEC;
  const bool col_ok = coff < a.d;
  float acc[VEC];

  if (bid < 0) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * GPB + g;
    if (t >= a.n_chunks) return;
    const int h = a.chunk_heavy[t];
    const int64_t r = a.heavy_rows[h];
    if (r < a.row_begin || r >= a.row_end) return;
    const int64_t k = t - a.heavy_cptr[h];
    const int64_t re = a.rowptr[r + 1];
    const int64_t e0 = a.rowptr[r] + k * a.chunk;
    const int64_t e1 = min(e0 + static_cast<int64_t>(a.chunk), re);
    masked_or_plain_sum<G, VEC, U, HAS_VAL, POL, MASK>(a, e0, e1, l, col_ok, acc, col0);
    if (col_ok) store_vec<VEC>(a.partial + t * a.d + coff, acc);
    return;
  }

  const int64_t r = a.row_begin + bid * GPB + g;
  if (r >= a.row_end) return;
  const int64_t e0 = a.rowptr[r];
  const int64_t e1 = a.rowptr[r + 1];
  if (a.heavy_threshold > 0 && e1 - e0 > a.heavy_threshold) return;  // split-plan row
  int32_t orow = 0;  // the ordered hop's Y row: one load per row, issued ahead of the gathers
  if constexpr (ORD) orow = a.out_row[r];
  if constexpr (PK)
    gather_sum<G, VEC, U, HAS_VAL, POL, false, TX, TY, true>(a, e0, e1, l, col_ok, acc, col0,
                                                             s_dict);
  else
    masked_or_plain_sum<G, VEC, U, HAS_VAL, POL, MASK>(a, e0, e1, l, col_ok, acc, col0);
  const int64_t yr = ORD ? static_cast<int64_t>(orow) : r;
  const float s = a.row_scale ? a.row_scale[r] : 1.f;
  finish_row<G, VEC, EX, (POL & kPolNtStore) != 0, TX, TY, !MASK>(a, r, yr, s, l, coff, col_ok,
                                                                   acc);
}

// Segmented variant for short rows (hgd_split_plan.flags & HGD_PLAN_SEGMENTED): a group owns
// G consecutive rows and walks their nonzeros as ONE flat stream [rowptr[r0], rowptr[r0+G]) in
// batches of G indices, so every gather batch is full whatever the row lengths, the row pointers
// and row scales of all G rows arrive in one coalesced load, and the accumulator is flushed
// (scale, epilogue, store) at each row boundary. Sums stay in edge order per row.
template <int G, int VEC, int U, bool HAS_VAL, int POL, bool EX, class TX = float, class TY = float>
__global__ __launch_bounds__(kBlock) void spmm_seg_kernel(SpmmArgsT<TX, TY> a) {
  constexpr int GPB = kBlock / G;
  const int g = threadIdx.x / G;
  const int l = threadIdx.x % G;
  const int64_t r0 = a.row_begin + (static_cast<int64_t>(blockIdx.x) * GPB + g) * G;
  if (r0 >= a.row_end) return;
  const int nr = static_cast<int>(min(static_cast<int64_t>(G), a.row_end - r0));
  int64_t my_end = 0;  // lane j: end of local row j
  float my_s = 1.f;    // lane j: scale of local row j
  if (l < nr) {
    my_end = a.rowptr[r0 + l + 1];
    if (a.row_scale) my_s = a.row_scale[r0 + l];
  }
  const int64_t e_begin = a.rowptr[r0];
  const int64_t e_end = __shfl(my_end, nr - 1, G);
  const int64_t coff = static_cast<int64_t>(a.col0) + static_cast<int64_t>(l) * VEC;
  const bool col_ok = coff < a.d;
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  int cur = 0;
  int64_t next_b = __shfl(my_end, 0, G);

  auto flush = [&]() {
    const float s = __shfl(my_s, cur, G);
    float y[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      y[i] = acc[i];
      acc[i] = 0.f;
    }
    finish_row<G, VEC, EX, (POL & kPolNtStore) != 0>(a, r0 + cur, r0 + cur, s, l, coff, col_ok,
                                                     y);
    ++cur;
    const int64_t nb = __shfl(my_end, cur < nr ? cur : 0, G);
    next_b = cur < nr ? nb : INT64_MAX;
  };

  constexpr bool PF = (POL & kPolPrefetch) != 0;
  int nxc = 0, unused_keep = 0;
  float nxw = 1.f;
  if constexpr (PF) {
    if (e_begin < e_end)
      load_index<HAS_VAL, POL>(
          a, e_begin, static_cast<int>(min(static_cast<int64_t>(G), e_end - e_begin)), l, nxc,
          nxw, unused_keep);
  }
  for (int64_t eb = e_begin; eb < e_end; eb += G) {
    const int n = static_cast<int>(min(static_cast<int64_t>(G), e_end - eb));
    int myc;
    float myw;
    if constexpr (PF) {
      myc = nxc;
      myw = nxw;
      const int64_t en = eb + G;
      if (en < e_end)
        load_index<HAS_VAL, POL>(
            a, en, static_cast<int>(min(static_cast<int64_t>(G), e_end - en)), l, nxc, nxw,
            unused_keep);
    } else {
      load_index<HAS_VAL, POL>(a, eb, n, l, myc, myw, unused_keep);
    }
    for (int k = 0; k < n; k += U) {
      float xv[U][VEC];
      float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = k + u;
        const int c = __shfl(myc, kk, G);
        if constexpr (HAS_VAL) w[u] = __shfl(myw, kk, G);
        if (kk < n && col_ok) {
          load_vec<VEC, (POL & kPolNtGather) != 0>(a.X + static_cast<int64_t>(c) * a.ldx + coff,
                                                   xv[u]);
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) xv[u][i] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < n) {
          const int64_t e = eb + k + u;
          while (e >= next_b) flush();  // group-uniform; also emits empty rows
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            if constexpr (HAS_VAL)
              acc[i] = fmaf(w[u], xv[u][i], acc[i]);
            else
              acc[i] += xv[u][i];
          }
        }
      }
    }
  }
  while (cur < nr) flush();
}

// One block per split row: each of the GPB lane groups sums the chunk partials
// t = first + g, first + g + GPB, ... (FU independent loads in flight), then group 0 adds the
// GPB group sums in group order. The combine order is fixed by (chunk count, GPB), so the result
// is deterministic run to run; a popular item with ~10^4 chunks is reduced by GPB·FU loads in
// flight instead of one serial chain.
template <int G, int VEC, bool EX, class TX = float, class TY = float>
__global__ __launch_bounds__(kBlock) void spmm_fixup_kernel(SpmmArgsT<TX, TY> a) {
  constexpr int GPB = kBlock / G;
  constexpr int FU = 4;
  __shared__ float s_acc[GPB][G * VEC];
  const int g = threadIdx.x / G;
  const int l = threadIdx.x % G;
  const int64_t h = blockIdx.x;
  const int64_t r = a.heavy_rows[h];
  if (r < a.row_begin || r >= a.row_end) return;  // block-uniform
  const int64_t coff = static_cast<int64_t>(a.col0) + static_cast<int64_t>(l) * VEC;
  const bool col_ok = coff < a.d;
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  const int64_t t0 = a.heavy_cptr[h], t1 = a.heavy_cptr[h + 1];
  for (int64_t t = t0 + g; t < t1; t += GPB * FU) {
    float v[FU][VEC];
#pragma unroll
    for (int u = 0; u < FU; ++u) {
      const int64_t tt = t + static_cast<int64_t>(u) * GPB;
      if (tt < t1 && col_ok) {
        load_vec<VEC>(a.partial + tt * a.d + coff, v[u]);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[u][i] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < FU; ++u)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += v[u][i];
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) s_acc[g][l * VEC + i] = acc[i];
  __syncthreads();
  if (g != 0) return;  // group 0 (all of its lanes: finish_row reduces over the group)
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = s_acc[0][l * VEC + i];
  if constexpr (EX && sizeof(TX) == 2) {
    // (the fused epilogue over a 16-bit table: the same sums in the same order, four groups at a
    // time — unrolled in full, a narrow group's GPB·VEC loads are all hoisted: 256 VGPRs at
    // d = 64 and private memory at d = 32)
#pragma unroll 4
    for (int k = 1; k < GPB; ++k)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += s_acc[k][l * VEC + i];
  } else {
    for (int k = 1; k < GPB; ++k)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += s_acc[k][l * VEC + i];
  }
  const float s = a.row_scale ? a.row_scale[r] : 1.f;
  finish_row<G, VEC, EX, false>(a, r, r, s, l, coff, col_ok, acc);
}

}  // namespace hgd
