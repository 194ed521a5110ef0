// CSR row-gather SpMM hop for gfx950 (CDNA4, wave64).
//
// Replaces torch.sparse.mm(adj, X) / torch.sparse.mm(adj.t(), X) (HCCF.py:199, HGNN_HD4.py:459-462,
// HGCN.py:173-175) and the torch_scatter mean pair (layers2/EquivSetConv2.py:88-93) of the
// reference (paths relative to /root/reference/HD_SELFRec).
//
// Work mapping (HBM-bound gather, ~0.5 flop/B; no MFMA):
//   * one row of Y per group of G lanes; each lane owns VEC contiguous columns, so a group moves
//     one gathered X row per load instruction (d=64: G=16 lanes × float4 = 256 B, 4 rows per wave);
//   * the group loads G column indices (and weights) with one coalesced load and broadcasts them
//     with __shfl, then issues U independent row gathers before consuming any of them, so every
//     lane keeps U×16 B in flight (U=8: 8 KB per wave at d=64);
//   * the sum runs in edge order in fp32 (single accumulator, fmaf), so results are deterministic;
//   * rows longer than the split plan's threshold are cut into fixed-size chunks handled by extra
//     blocks placed FIRST in the grid (they are the longest work items); a fix-up kernel sums the
//     chunk partials in chunk order — no float atomics anywhere.
// The kernels are spmm_kernels.h's; the host side (argument checks, pass plan, launch chain) is
// spmm_launch.h's, shared with spmm_dt.hip. This file holds the fp32 entry points and the
// column-block builder of the source-blocked hop.
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "spmm_launch.h"

extern "C" size_t hgd_spmm_workspace_size(const hgd_split_plan* plan, int32_t d) {
  if (!plan || plan->n_heavy <= 0 || plan->threshold <= 0 || d <= 0) return 0;
  return hgd::align_up(static_cast<size_t>(plan->n_chunks) * static_cast<size_t>(d) * 4);
}

namespace hgd {
namespace {

// Source block of column c among n_blk ranges [⌊n_cols·k/n_blk⌋, ⌊n_cols·(k+1)/n_blk⌋), stepping
// k up from the previous nonzero's block (the columns of a row ascend).
__device__ __forceinline__ int32_t advance_block(int64_t c, int32_t k, int64_t n_cols,
                                                 int32_t n_blk) {
  while (k + 1 < n_blk && c >= n_cols * (k + 1) / n_blk) ++k;
  return k;
}

// cnt[k·n_rows + r] = nonzeros of row r in source block k (block-major, the order of the blocked
// copy); one thread per row walks it once. cnt[n_blk·n_rows] = 0 closes the scan.
__global__ void col_block_count_kernel(const int64_t* __restrict__ rowptr,
                                       const int32_t* __restrict__ col, int64_t n_rows,
                                       int64_t n_cols, int32_t n_blk, int64_t* __restrict__ cnt) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r == 0) cnt[static_cast<int64_t>(n_blk) * n_rows] = 0;
  if (r >= n_rows) return;
  const int64_t b = rowptr[r], e = rowptr[r + 1];
  int32_t k = 0;
  int64_t start = b;
  for (int64_t i = b; i < e; ++i) {
    const int32_t kk = advance_block(col[i], k, n_cols, n_blk);
    if (kk != k) {
      cnt[static_cast<int64_t>(k) * n_rows + r] = i - start;
      for (int32_t j = k + 1; j < kk; ++j) cnt[static_cast<int64_t>(j) * n_rows + r] = 0;
      k = kk;
      start = i;
    }
  }
  cnt[static_cast<int64_t>(k) * n_rows + r] = e - start;
  for (int32_t j = k + 1; j < n_blk; ++j) cnt[static_cast<int64_t>(j) * n_rows + r] = 0;
}

// Moves every nonzero to its block-major position blk_start[k·n_rows + r] + (its rank inside the
// row's block k): blk_col gets the column, blk_perm (optional) the source position, with which
// any per-nonzero array of the structure is gathered into the same order.
__global__ void col_block_scatter_kernel(const int64_t* __restrict__ rowptr,
                                         const int32_t* __restrict__ col, int64_t n_rows,
                                         int64_t n_cols, int32_t n_blk,
                                         const int64_t* __restrict__ blk_start,
                                         int32_t* __restrict__ blk_col,
                                         int32_t* __restrict__ blk_perm) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const int64_t b = rowptr[r], e = rowptr[r + 1];
  int32_t k = 0;
  int64_t start = b, out = blk_start[r];
  for (int64_t i = b; i < e; ++i) {
    const int32_t c = col[i];
    const int32_t kk = advance_block(c, k, n_cols, n_blk);
    if (kk != k) {
      k = kk;
      start = i;
      out = blk_start[static_cast<int64_t>(k) * n_rows + r];
    }
    blk_col[out + (i - start)] = c;
    if (blk_perm) blk_perm[out + (i - start)] = static_cast<int32_t>(i);
  }
}

// Row order (hgd_spmm_row_order): a group of kOrdG lanes per row, kBlock / kOrdG rows per block.
constexpr int kOrdG = 16;

// key[r] = the smallest column of row r (its columns need not ascend), n_cols for an empty row.
__global__ __launch_bounds__(kBlock) void row_min_key_kernel(const int64_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ col,
                                                             int64_t n_rows, int32_t n_cols,
                                                             int32_t* __restrict__ key) {
  const int l = threadIdx.x % kOrdG;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kBlock / kOrdG) + threadIdx.x / kOrdG;
  if (r >= n_rows) return;  // group-uniform
  const int64_t b = rowptr[r], e = rowptr[r + 1];
  int32_t m = n_cols;
  for (int64_t i = b + l; i < e; i += kOrdG) m = min(m, col[i]);
#pragma unroll
  for (int w = kOrdG / 2; w >= 1; w >>= 1) m = min(m, __shfl_xor(m, w, kOrdG));
  if (l == 0) key[r] = m;
}

// len[p] = length of the row at position p; len[n_rows] = 0 closes the scan.
__global__ void row_order_len_kernel(const int64_t* __restrict__ rowptr,
                                     const int32_t* __restrict__ order, int64_t n_rows,
                                     int64_t* __restrict__ len) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p > n_rows) return;
  int64_t n = 0;
  if (p < n_rows) {
    const int64_t r = order[p];
    n = rowptr[r + 1] - rowptr[r];
  }
  len[p] = n;
}

// Copies row order[p] to position p: its columns, in their own order, and their source positions.
__global__ __launch_bounds__(kBlock) void row_order_copy_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ order, const int64_t* __restrict__ rowptr_o, int64_t n_rows,
    int32_t* __restrict__ col_o, int32_t* __restrict__ perm) {
  const int l = threadIdx.x % kOrdG;
  const int64_t p = static_cast<int64_t>(blockIdx.x) * (kBlock / kOrdG) + threadIdx.x / kOrdG;
  if (p >= n_rows) return;
  const int64_t r = order[p];
  const int64_t src = rowptr[r], n = rowptr[r + 1] - src, dst = rowptr_o[p];
  for (int64_t i = l; i < n; i += kOrdG) {
    col_o[dst + i] = col[src + i];
    perm[dst + i] = static_cast<int32_t>(src + i);
  }
}

// workspace of hgd_spmm_row_order: keys, sorted keys, permuted lengths, then the sort's and the
// scan's own (one after the other in the same tail)
struct RowOrderWs {
  size_t keys, keys_s, len, tail, total;
};

RowOrderWs row_order_ws(int64_t n_rows) {
  RowOrderWs w{};
  size_t scan = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan, static_cast<const int64_t*>(nullptr),
                                       static_cast<int64_t*>(nullptr), n_rows + 1) != hipSuccess)
    return w;
  const size_t sort = hgd_sort_perm_workspace_size(n_rows);
  if (sort == 0) return w;
  const size_t k = align_up(static_cast<size_t>(n_rows) * sizeof(int32_t));
  w.keys = 0;
  w.keys_s = k;
  w.len = 2 * k;
  w.tail = w.len + align_up(static_cast<size_t>(n_rows + 1) * sizeof(int64_t));
  w.total = w.tail + (sort > align_up(scan) ? sort : align_up(scan));
  return w;
}

// Block order (hgd_spmm_col_blocks_ordered): dest[k·n_rows + out_row[k·n_rows + p]] =
// blk_start[k·n_rows + p], where row r's piece of block k starts in the ordered copy — the start
// array col_block_scatter_kernel moves the nonzeros by. n = n_blk·n_rows.
__global__ void block_order_dest_kernel(const int64_t* __restrict__ blk_start,
                                        const int32_t* __restrict__ out_row, int64_t n_rows,
                                        int64_t n, int64_t* __restrict__ dest) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dest[i - i % n_rows + out_row[i]] = blk_start[i];
}

// Packed entries (hgd_spmm_pack_entries): one thread per nonzero e of the block-major copy. Its
// block is the k with bound[k] <= e < bound[k + 1] over the n_blk + 1 block boundaries
// bound[k] = blk_start[k·n_rows] (read once per workgroup; an empty block has two equal bounds and
// is skipped); the word is the column counted from the block's first source row beside the code
// of the source row.
__global__ __launch_bounds__(kBlock) void pack_entries_kernel(
    const int64_t* __restrict__ blk_start, const int32_t* __restrict__ blk_col,
    const int32_t* __restrict__ src_code, int64_t n_rows, int64_t n_src_rows, int64_t nnz,
    int32_t n_blk, int32_t idx_bits, uint32_t* __restrict__ ent) {
  __shared__ int64_t bound[65];  // (n_blk <= 64)
  if (static_cast<int32_t>(threadIdx.x) <= n_blk)
    bound[threadIdx.x] = blk_start[static_cast<int64_t>(threadIdx.x) * n_rows];
  __syncthreads();
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= nnz) return;
  int32_t k = 0;
  while (k + 1 < n_blk && e >= bound[k + 1]) ++k;
  const int32_t c = blk_col[e];
  const int64_t base = n_src_rows * k / n_blk;
  ent[e] = static_cast<uint32_t>(c - base) | static_cast<uint32_t>(src_code[c]) << idx_bits;
}

// workspace of hgd_spmm_col_blocks_ordered: the block-major counts (then the permuted lengths),
// the natural block-major starts (then the scatter's destinations), one block's keys and sorted
// keys, then the sort's and the scan's own (one after the other in the same tail)
struct BlockOrderWs {
  size_t cnt, start, keys, keys_s, tail, total;
};

BlockOrderWs block_order_ws(int64_t n_rows, int32_t n_blk) {
  BlockOrderWs w{};
  const int64_t n = static_cast<int64_t>(n_blk) * n_rows + 1;
  size_t scan = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan, static_cast<const int64_t*>(nullptr),
                                       static_cast<int64_t*>(nullptr), n) != hipSuccess)
    return w;
  const size_t sort = hgd_sort_perm_workspace_size(n_rows);
  if (sort == 0) return w;
  const size_t a = align_up(static_cast<size_t>(n) * sizeof(int64_t));
  const size_t k = align_up(static_cast<size_t>(n_rows) * sizeof(int32_t));
  w.cnt = 0;
  w.start = a;
  w.keys = 2 * a;
  w.keys_s = w.keys + k;
  w.tail = w.keys_s + k;
  w.total = w.tail + (sort > align_up(scan) ? sort : align_up(scan));
  return w;
}

// Permutation check of a caller's order (hgd_spmm_row_order_from, hgd_spmm_col_blocks_ordered_from):
// flag[k·n_rows + order[k·n_rows + p]] = 1 for every entry inside [0, n_rows) — plain stores of the
// same value, no atomics — so the flags sum to n = n_blk·n_rows exactly when every block's order
// is a permutation.
__global__ void order_flag_kernel(const int32_t* __restrict__ order, int64_t n_rows, int64_t n,
                                  int32_t* __restrict__ flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = order[i];
  if (r >= 0 && r < n_rows) flag[i - i % n_rows + r] = 1;
}

struct WidenFlag {
  __host__ __device__ int64_t operator()(int32_t f) const { return f; }
};
using FlagIter = hipcub::TransformInputIterator<int64_t, WidenFlag, const int32_t*>;

// what the check needs behind a builder's own workspace: the sum, then the reduction's own
size_t order_check_ws(int64_t n) {
  size_t red = 0;
  if (hipcub::DeviceReduce::Sum(nullptr, red, FlagIter(nullptr, WidenFlag{}),
                                static_cast<int64_t*>(nullptr), n) != hipSuccess)
    return 0;
  return 256 + align_up(red > 0 ? red : 1);
}

// Whether order [n] is n / n_rows permutations of [0, n_rows), one after the other. flag: int32 [n]
// of scratch; tail: order_check_ws(n) bytes. Waits for the stream (the caller built the order on
// the host: it has synchronised already), so nothing reads the structure through a bad order.
hgd_status check_order(const char* fn, const int32_t* order, int64_t n_rows, int64_t n,
                       int32_t* flag, char* tail, size_t tail_bytes, hipStream_t st) {
  HGD_HIP(hipMemsetAsync(flag, 0, static_cast<size_t>(n) * sizeof(int32_t), st));
  hipLaunchKernelGGL(order_flag_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, order, n_rows, n,
                     flag);
  hgd_status s = check_launch(fn, "order flags");
  if (s != HGD_OK) return s;
  int64_t* sum = reinterpret_cast<int64_t*>(tail);
  size_t red_bytes = tail_bytes - 256;
  HGD_HIP(hipcub::DeviceReduce::Sum(tail + 256, red_bytes, FlagIter(flag, WidenFlag{}), sum, n, st));
  int64_t got = -1;
  HGD_HIP(hipMemcpyAsync(&got, sum, sizeof(got), hipMemcpyDeviceToHost, st));
  HGD_HIP(hipStreamSynchronize(st));
  if (got != n)
    return fail(HGD_ERR_INVALID_ARG, "%s: the order is not a permutation of the rows (%lld of %lld "
                "rows named)", fn, (long long)got, (long long)n);
  return HGD_OK;
}

// hgd_spmm_row_order's steps after its sort, over any order: permuted lengths, scan, copy of the
// columns and their source positions. len / tail: RowOrderWs's.
hgd_status row_order_tail(const char* fn, const int64_t* rowptr, const int32_t* col,
                          const int32_t* order, int64_t n_rows, int64_t* rowptr_o, int32_t* col_o,
                          int32_t* perm, int64_t* len, char* tail, size_t tail_bytes,
                          hipStream_t st) {
  constexpr int kRowsPerBlock = kBlock / kOrdG;
  const int64_t grid = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
  hipLaunchKernelGGL(row_order_len_kernel, dim3(grid_for(n_rows + 1)), dim3(kBlock), 0, st, rowptr,
                     order, n_rows, len);
  hgd_status s = check_launch(fn, "lengths");
  if (s != HGD_OK) return s;
  HGD_HIP(hipcub::DeviceScan::ExclusiveSum(tail, tail_bytes, len, rowptr_o, n_rows + 1, st));
  hipLaunchKernelGGL(row_order_copy_kernel, dim3(grid), dim3(kBlock), 0, st, rowptr, col, order,
                     rowptr_o, n_rows, col_o, perm);
  return check_launch(fn, "copy");
}

// hgd_spmm_col_blocks_ordered's steps after its sorts, over any per-block orders blk_out_row:
// permuted lengths per block, one scan, every piece's destination, the scatter. start: the natural
// block-major starts (hgd_spmm_col_blocks' count and scan), then the destinations; cnt: scratch
// of the same size.
hgd_status block_order_tail(const char* fn, const int64_t* rowptr, const int32_t* col,
                            int64_t n_rows, int64_t n_cols, int32_t n_blocks, int64_t* blk_start,
                            int32_t* blk_col, int32_t* blk_perm, const int32_t* blk_out_row,
                            int64_t* cnt, int64_t* start, char* tail, size_t tail_bytes,
                            hipStream_t st) {
  const int64_t n = static_cast<int64_t>(n_blocks) * n_rows;
  const int64_t row_grid = (n_rows + 255) / 256;
  hgd_status s;
  for (int32_t k = 0; k < n_blocks; ++k) {
    const int64_t off = static_cast<int64_t>(k) * n_rows;
    // (writes the closing 0 at cnt[off + n_rows], which the next block's launch overwrites)
    hipLaunchKernelGGL(row_order_len_kernel, dim3(grid_for(n_rows + 1)), dim3(kBlock), 0, st,
                       start + off, blk_out_row + off, n_rows, cnt + off);
    s = check_launch(fn, "lengths");
    if (s != HGD_OK) return s;
  }
  HGD_HIP(hipcub::DeviceScan::ExclusiveSum(tail, tail_bytes, cnt, blk_start, n + 1, st));
  // every piece's start in the ordered copy, indexed by (block, row), and the nonzeros moved
  // there from the source structure: blk_perm is their source position as in hgd_spmm_col_blocks
  hipLaunchKernelGGL(block_order_dest_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, blk_start,
                     blk_out_row, n_rows, n, start);
  s = check_launch(fn, "destinations");
  if (s != HGD_OK) return s;
  hipLaunchKernelGGL(col_block_scatter_kernel, dim3(row_grid), dim3(256), 0, st, rowptr, col,
                     n_rows, n_cols, n_blocks, start, blk_col, blk_perm);
  return check_launch(fn, "ordered scatter");
}

}  // namespace
}  // namespace hgd

extern "C" size_t hgd_spmm_row_order_workspace_size(int64_t n_rows) {
  if (n_rows <= 0 || n_rows >= 0x7fffffffLL) return 0;
  return hgd::row_order_ws(n_rows).total;
}

extern "C" hgd_status hgd_spmm_row_order(const int64_t* rowptr, const int32_t* col,
                                         int64_t n_rows, int64_t n_cols, int32_t* order,
                                         int64_t* rowptr_o, int32_t* col_o, int32_t* perm,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  using namespace hgd;
  clear_error();
  HGD_REQUIRE(n_rows >= 0 && n_cols >= 0, "hgd_spmm_row_order: negative sizes");
  HGD_REQUIRE(n_rows < 0x7fffffffLL, "hgd_spmm_row_order: n_rows >= 2^31 - 1");
  HGD_REQUIRE(n_cols < 0x7fffffffLL, "hgd_spmm_row_order: n_cols >= 2^31 - 1");
  if (n_rows == 0) return HGD_OK;
  HGD_REQUIRE(rowptr && order && rowptr_o, "hgd_spmm_row_order: null rowptr / order / rowptr_o");
  const RowOrderWs w = row_order_ws(n_rows);
  if (w.total == 0 || !workspace || workspace_bytes < w.total)
    return fail(HGD_ERR_WORKSPACE, "hgd_spmm_row_order: workspace %zu < %zu", workspace_bytes,
                w.total);
  constexpr int kRowsPerBlock = kBlock / kOrdG;
  const int64_t grid = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
  HGD_REQUIRE(grid <= 0x7fffffffLL, "hgd_spmm_row_order: too many rows");
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  int32_t* keys = reinterpret_cast<int32_t*>(ws + w.keys);
  int32_t* keys_s = reinterpret_cast<int32_t*>(ws + w.keys_s);
  int64_t* len = reinterpret_cast<int64_t*>(ws + w.len);
  hipLaunchKernelGGL(row_min_key_kernel, dim3(grid), dim3(kBlock), 0, st, rowptr, col, n_rows,
                     static_cast<int32_t>(n_cols), keys);
  hgd_status s = check_launch("hgd_spmm_row_order", "keys");
  if (s != HGD_OK) return s;
  // stable: rows with the same smallest column stay in natural order
  s = hgd_sort_perm(keys, n_rows, n_cols + 1, keys_s, order, ws + w.tail, workspace_bytes - w.tail,
                    stream);
  if (s != HGD_OK) return s;
  return row_order_tail("hgd_spmm_row_order", rowptr, col, order, n_rows, rowptr_o, col_o, perm,
                        len, ws + w.tail, workspace_bytes - w.tail, st);
}

extern "C" size_t hgd_spmm_row_order_from_workspace_size(int64_t n_rows) {
  if (n_rows <= 0 || n_rows >= 0x7fffffffLL) return 0;
  const size_t own = hgd::row_order_ws(n_rows).total, check = hgd::order_check_ws(n_rows);
  return own && check ? own + check : 0;
}

extern "C" hgd_status hgd_spmm_row_order_from(const int32_t* order, const int64_t* rowptr,
                                              const int32_t* col, int64_t n_rows, int64_t n_cols,
                                              int64_t* rowptr_o, int32_t* col_o, int32_t* perm,
                                              void* workspace, size_t workspace_bytes,
                                              void* stream) {
  using namespace hgd;
  clear_error();
  constexpr const char* fn = "hgd_spmm_row_order_from";
  HGD_REQUIRE(n_rows >= 0 && n_cols >= 0, "%s: negative sizes", fn);
  HGD_REQUIRE(n_rows < 0x7fffffffLL, "%s: n_rows >= 2^31 - 1", fn);
  HGD_REQUIRE(n_cols < 0x7fffffffLL, "%s: n_cols >= 2^31 - 1", fn);
  if (n_rows == 0) return HGD_OK;
  HGD_REQUIRE(rowptr && order && rowptr_o, "%s: null rowptr / order / rowptr_o", fn);
  const RowOrderWs w = row_order_ws(n_rows);
  const size_t need = hgd_spmm_row_order_from_workspace_size(n_rows);
  if (need == 0 || !workspace || workspace_bytes < need)
    return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < %zu", fn, workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  // (the flags where the builder's keys would be; the check's own behind the builder's workspace)
  hgd_status s = check_order(fn, order, n_rows, n_rows, reinterpret_cast<int32_t*>(ws + w.keys),
                             ws + w.total, need - w.total, st);
  if (s != HGD_OK) return s;
  return row_order_tail(fn, rowptr, col, order, n_rows, rowptr_o, col_o, perm,
                        reinterpret_cast<int64_t*>(ws + w.len), ws + w.tail, w.total - w.tail, st);
}

namespace hgd {
namespace {

// The rows per workgroup and the window of the hop of one form (sx / sy: the element sizes of X
// and Y; fused: with a row epilogue, which has no LayerNorm here: the plan of a row of any
// width), from the launcher's own pass plan over 16-byte aligned rows of d (a blocked hop: any
// block count).
int32_t order_geometry(const char* fn, int32_t d, int32_t blocked, size_t sx, size_t sy,
                       bool fused, int32_t* rows_per_wg, int64_t* window) {
  if (d <= 0 || !rows_per_wg || !window) return 0;
  SpmmRequest r{fn, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0,
                nullptr, d, nullptr, d, d, HGD_EPI_NONE, 0.f};
  r.blocked = blocked != 0;
  r.n_blk = blocked ? 2 : 0;
  const hgd_row_epilogue ex{};
  if (fused) r.ex = &ex;
  SpmmPassPlan p;
  if (spmm_pass_plan(r, sx, sy, &p) != HGD_OK) return 0;
  *rows_per_wg = kBlock / p.G;
  // the gathers an XCD's 4 MiB of L2 holds: one is a pass's piece of a source row
  const int64_t piece = static_cast<int64_t>(d < p.step ? d : p.step) * static_cast<int64_t>(sx);
  *window = (int64_t(4) << 20) / piece;
  return 1;
}

}  // namespace
}  // namespace hgd

extern "C" int32_t hgd_spmm_order_geometry(int32_t d, int32_t blocked, int32_t* rows_per_wg,
                                           int64_t* window) {
  return hgd::order_geometry("hgd_spmm_order_geometry", d, blocked, 4, 4, false, rows_per_wg,
                             window);
}

extern "C" int32_t hgd_spmm_order_geometry_dt(int32_t d, int32_t blocked, int32_t x_dtype,
                                              int32_t y_dtype, int32_t fused,
                                              int32_t* rows_per_wg, int64_t* window) {
  const bool xb = x_dtype == HGD_DT_BF16, yb = y_dtype == HGD_DT_BF16;
  if ((!xb && x_dtype != HGD_DT_F32) || (!yb && y_dtype != HGD_DT_F32)) return 0;
  // no such hop: a fused row epilogue into a 16-bit Y, or over source blocks
  if (fused && (yb || blocked)) return 0;
  return hgd::order_geometry("hgd_spmm_order_geometry_dt", d, blocked, xb ? 2 : 4, yb ? 2 : 4,
                             fused != 0, rows_per_wg, window);
}

extern "C" int32_t hgd_spmm_row_order_kind_for(int64_t n_rows, int64_t n_src_rows, int64_t nnz,
                                               int32_t d, int32_t n_blocks) {
  // the greedy order wherever a size rule orders the hop (a blocked one: each block's rows)
  const int32_t on = n_blocks > 1 ? hgd_spmm_block_order_for(n_rows, n_src_rows, nnz, d, n_blocks)
                                  : hgd_spmm_row_order_for(n_rows, n_src_rows, nnz, d);
  return on ? HGD_ORDER_GREEDY : HGD_ORDER_NONE;
}

extern "C" int32_t hgd_spmm_row_order_for(int64_t n_rows, int64_t n_src_rows, int64_t nnz,
                                          int32_t d) {
  if (n_rows <= 0 || n_src_rows <= 0 || nnz <= 0 || d <= 0) return 0;
  // the table one pass gathers from (rows wider than 128 run as 64-column passes): one that fits
  // the aggregate L2 (8 XCDs × 4 MiB) is served from it in any order
  const double table = static_cast<double>(n_src_rows) * (d <= 128 ? d : 64) * 4.0;
  if (table < 33554432.0) return 0;
  // the order turns about one gather per row: nothing to gain on long rows
  if (nnz > 32 * n_rows) return 0;
  // between the two bounds it is on: at 10 M users × 1 M items × 100 M edges the ordered hop into
  // users is 7–8 % faster at d = 32, 64 and 128 (scripts/bench_row_order.py)
  return 1;
}

extern "C" int32_t hgd_spmm_row_order_for_dt(int64_t n_rows, int64_t n_src_rows, int64_t nnz,
                                             int32_t d, int32_t x_dtype, int32_t y_dtype,
                                             int32_t fused, int32_t masked) {
  const bool xb = x_dtype == HGD_DT_BF16, yb = y_dtype == HGD_DT_BF16;
  if ((!xb && x_dtype != HGD_DT_F32) || (!yb && y_dtype != HGD_DT_F32)) return 0;
  if (!xb && !yb && !fused && !masked)  // the plain fp32 hop: its own rule
    return hgd_spmm_row_order_for(n_rows, n_src_rows, nnz, d);
  // The fused, masked and 16-bit forms are ordered only where the ordered twin beat the unordered
  // call by more than the rounds' ranges, in both orders a host may pick (min column, greedy).
  // Measured on MI355X over the bench graph's hop into users, 10 M users × 1 M items × 100 M
  // edges, 5 interleaved rounds of 10 calls, ranges 0.002–0.04 ms
  // (scripts/bench_ordered_forms.py, profiles/ordered_forms/):
  //   fused fp32 (LayerNorm + residual), d = 128: 9.09 → 8.89 ms min column (−2.2 %), 9.31 → 8.86
  //     greedy (−4.8 %); the LocalAwareEncoder at the Amazon-Book shape, fwd + bwd: −0.5 / −0.6 /
  //     −0.9 % on three repeats. At d = 64 it loses: +2.7 % min column, +1.4 % greedy;
  //   plain bf16 → bf16 hop, d = 128: 6.51 → 6.20 ms min column (−4.8 %), 6.43 → 6.03 greedy
  //     (−6.2 %). At d = 64 the greedy order gains 5.7 % and the min-column order 0.7 %, inside
  //     the ranges: a rule cannot see which of the two its host walks, so it stays off;
  //   fused bf16: +9.5 / +7.4 % at d = 64, +1.6 % (min column) / −1.3 % (greedy) at d = 128: off;
  //   every masked form loses 3–13 % with the per-step gather of its mask counted: off.
  // So: the two forms that won, at the width they won at, inside the plain rule's two bounds
  // (the table one pass gathers from, in the form's element size, against the aggregate L2; the
  // average row length). Everything else, unmeasured widths and dtype pairs included, answers 0
  // and is reachable through HGD_SPMM_ROW_ORDER=1 in the Python host, as the blocked bf16 hop is
  // through HGD_SPMM_BLOCKS.
  if (n_rows <= 0 || n_src_rows <= 0 || nnz <= 0 || masked || d != 128) return 0;
  const bool fused_f32 = fused && !xb && !yb, plain_bf16 = !fused && xb && yb;
  if (!fused_f32 && !plain_bf16) return 0;
  const double table = static_cast<double>(n_src_rows) * d * (xb ? 2.0 : 4.0);
  if (table < 33554432.0) return 0;
  return nnz > 32 * n_rows ? 0 : 1;
}

extern "C" int32_t hgd_spmm_block_order_for(int64_t n_rows, int64_t n_src_rows, int64_t nnz,
                                            int32_t d, int32_t n_blocks) {
  if (n_rows <= 0 || n_src_rows <= 0 || nnz <= 0 || d <= 0 || n_blocks <= 0) return 0;
  // hgd_spmm_row_order_for's two bounds applied to one source block: the slice one pass gathers
  // from (a blocked hop runs rows wider than 128 as 128-column passes) fits the aggregate L2 ...
  const double slice =
      static_cast<double>(n_src_rows) / n_blocks * (d < 128 ? d : 128) * 4.0;
  if (slice < 33554432.0) return 0;
  // ... or the order turns one gather of a long piece
  if (nnz > 32 * static_cast<int64_t>(n_blocks) * n_rows) return 0;
  // between the two bounds it is on: at 10 M users × 1 M items × 100 M edges the hop into items
  // is 1.4 % faster at d = 64 (P = 4) and 3.9 % at d = 128 (P = 8), with 2.4 % less fetched at
  // d = 64 (scripts/bench_mall_blocked.py --block-order both)
  return 1;
}

extern "C" hgd_status hgd_spmm_ordered(const int64_t* rowptr, const int32_t* col,
                                       const float* val, const float* row_scale, int64_t n_rows,
                                       int64_t n_src_rows, int64_t row_begin, int64_t row_end,
                                       const float* X, int64_t ldx, float* Y, int64_t ldy,
                                       int32_t d, int32_t epilogue, float slope,
                                       const hgd_split_plan* plan, void* workspace,
                                       size_t workspace_bytes, const int32_t* out_row,
                                       void* stream) {
  hgd::clear_error();
  hgd::SpmmRequest r{"hgd_spmm_ordered", rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                     row_end, X, ldx, Y, ldy, d, epilogue, slope, plan, workspace, workspace_bytes,
                     stream};
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" hgd_status hgd_spmm(const int64_t* rowptr, const int32_t* col, const float* val,
                               const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                               int64_t row_begin, int64_t row_end, const float* X, int64_t ldx,
                               float* Y, int64_t ldy, int32_t d, int32_t epilogue, float slope,
                               const hgd_split_plan* plan, void* workspace,
                               size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  hgd::SpmmRequest r{"hgd_spmm", rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                     row_end, X, ldx, Y, ldy, d, epilogue, slope, plan, workspace, workspace_bytes,
                     stream};
  return hgd::spmm_launch<float, float>(r);
}

extern "C" int32_t hgd_spmm_blocks_for(int64_t n_src_rows, int32_t d) {
  // one pass's gathered table: a blocked hop runs rows wider than 128 as 128-column passes
  const double table = static_cast<double>(n_src_rows) * (d < 128 ? d : 128) * 4.0;
  if (n_src_rows <= 0 || d <= 0 || table < 536870912.0) return 0;  // < 512 MiB: one pass
  if (table < 1073741824.0) return 2;                               // < 1 GiB: two blocks
  const double x = table / (640.0 * 1048576.0);                     // ~ one per 640 MiB
  double p = std::floor(x);  // rounded half to even
  const double frac = x - p;
  if (frac > 0.5 || (frac == 0.5 && std::fmod(p, 2.0) != 0.0)) p += 1.0;
  return static_cast<int32_t>(p < 4.0 ? 4.0 : (p > 16.0 ? 16.0 : p));
}

extern "C" size_t hgd_spmm_col_blocks_workspace_size(int64_t n_rows, int32_t n_blocks) {
  if (n_rows <= 0 || n_blocks <= 0) return 0;
  const int64_t n = static_cast<int64_t>(n_blocks) * n_rows + 1;
  size_t scan = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan, static_cast<const int64_t*>(nullptr),
                                       static_cast<int64_t*>(nullptr), n) != hipSuccess)
    return 0;
  return hgd::align_up(static_cast<size_t>(n) * sizeof(int64_t)) + hgd::align_up(scan);
}

extern "C" hgd_status hgd_spmm_col_blocks(const int64_t* rowptr, const int32_t* col,
                                          int64_t n_rows, int64_t n_cols, int32_t n_blocks,
                                          int64_t* blk_start, int32_t* blk_col,
                                          int32_t* blk_perm, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  using namespace hgd;
  clear_error();
  HGD_REQUIRE(n_rows >= 0 && n_cols >= 0, "hgd_spmm_col_blocks: negative sizes");
  HGD_REQUIRE(n_blocks >= 1 && n_blocks <= 64, "hgd_spmm_col_blocks: blocks must be 1..64");
  HGD_REQUIRE(n_cols < (int64_t(1) << 31), "hgd_spmm_col_blocks: n_cols >= 2^31");
  if (n_rows == 0) return HGD_OK;
  HGD_REQUIRE(rowptr && blk_start, "hgd_spmm_col_blocks: null rowptr / blk_start");
  const size_t need = hgd_spmm_col_blocks_workspace_size(n_rows, n_blocks);
  if (!workspace || workspace_bytes < need)
    return fail(HGD_ERR_WORKSPACE, "hgd_spmm_col_blocks: workspace %zu < %zu", workspace_bytes,
                need);
  const int64_t grid = (n_rows + 255) / 256;
  HGD_REQUIRE(grid <= 0x7fffffffLL, "hgd_spmm_col_blocks: too many rows");
  hipStream_t st = as_stream(stream);
  const int64_t n = static_cast<int64_t>(n_blocks) * n_rows + 1;
  int64_t* cnt = static_cast<int64_t*>(workspace);
  char* tmp = static_cast<char*>(workspace) + align_up(static_cast<size_t>(n) * sizeof(int64_t));
  size_t tmp_bytes = workspace_bytes - align_up(static_cast<size_t>(n) * sizeof(int64_t));
  hipLaunchKernelGGL(col_block_count_kernel, dim3(grid), dim3(256), 0, st, rowptr, col, n_rows,
                     n_cols, n_blocks, cnt);
  hgd_status s = check_launch("hgd_spmm_col_blocks count");
  if (s != HGD_OK) return s;
  HGD_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, blk_start, n, st));
  hipLaunchKernelGGL(col_block_scatter_kernel, dim3(grid), dim3(256), 0, st, rowptr, col, n_rows,
                     n_cols, n_blocks, blk_start, blk_col, blk_perm);
  return check_launch("hgd_spmm_col_blocks scatter");
}

extern "C" hgd_status hgd_spmm_blocked(const int64_t* blk_start, const int32_t* blk_col,
                                       const float* blk_val, const float* row_scale,
                                       int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                       int64_t row_end, const float* X, int64_t ldx, float* Y,
                                       int64_t ldy, int32_t d, int32_t epilogue, float slope,
                                       int32_t n_blocks, void* stream) {
  hgd::clear_error();
  hgd::SpmmRequest r{"hgd_spmm_blocked", nullptr, blk_col, blk_val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, epilogue, slope};
  r.blocked = true;
  r.blk_start = blk_start;
  r.n_blk = n_blocks;
  r.stream = stream;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" size_t hgd_spmm_blocked_split_workspace_size(const hgd_split_plan* plans,
                                                        int32_t n_blocks, int32_t d) {
  if (!plans || n_blocks < 1 || n_blocks > 64) return 0;
  size_t need = 0;  // the blocks run in stream order: the largest block's partials
  for (int32_t k = 0; k < n_blocks; ++k) {
    const size_t nk = hgd_spmm_workspace_size(plans + k, d);
    need = nk > need ? nk : need;
  }
  return need;
}

extern "C" hgd_status hgd_spmm_blocked_split(const int64_t* blk_start, const int32_t* blk_col,
                                             const float* blk_val, const float* row_scale,
                                             int64_t n_rows, int64_t n_src_rows,
                                             int64_t row_begin, int64_t row_end, const float* X,
                                             int64_t ldx, float* Y, int64_t ldy, int32_t d,
                                             int32_t epilogue, float slope, int32_t n_blocks,
                                             const hgd_split_plan* plans, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  // (the block count first: it says how many plans there are to read)
  HGD_REQUIRE(plans || n_blocks < 1 || n_blocks > 64, "hgd_spmm_blocked_split: null plans");
  hgd::SpmmRequest r{"hgd_spmm_blocked_split", nullptr, blk_col, blk_val, row_scale, n_rows,
                     n_src_rows, row_begin, row_end, X, ldx, Y, ldy, d, epilogue, slope};
  r.blocked = true;
  r.blk_start = blk_start;
  r.n_blk = n_blocks;
  r.blk_plans = plans;
  r.workspace = workspace;
  r.workspace_bytes = workspace_bytes;
  r.stream = stream;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" int32_t hgd_spmm_blocks_split_for(int64_t n_src_rows, int32_t d, int64_t nnz,
                                             int64_t n_chunks, int32_t chunk) {
  if (n_src_rows <= 0 || d <= 0 || nnz <= 0 || n_chunks <= 0 || chunk <= 0) return 0;
  // Measured on MI355X over the hop into items at 10 M users × 1 M items × 100 M draws, split at
  // 2048 into chunks of 512, against the plain split hop, interleaved, two repeats of five rounds
  // (scripts/bench_mall_blocked.py --zipf, profiles/blocked_split/):
  //   items ∝ rank^-0.8 (28.6 % of the nonzeros in split rows), d = 64: 4.10 / 4.09 ms plain,
  //     3.995 / 3.991 at P = 4 (−2.5 %, the rounds' ranges 0.02–0.05 ms), 4.00 / 4.01 at P = 2,
  //     4.65 at P = 8;
  //   the same at d = 128 (a 5.12 GB table): no block count beyond the plain hop's range;
  //   items ∝ rank^-1 (60.1 % in split rows): −0.8 / −1.3 % at d = 64 with P = 2, inside the
  //     plain hop's range on one repeat, nothing at d = 128; P = 8 is 7–24 % slower.
  // So the rule is on exactly where a block count won on both repeats, without a margin: four
  // blocks for a pass's gathered table (a blocked hop runs rows wider than 128 as 128-column
  // passes) from the 2.56 GB that won to below the 5.12 GB that did not, with at most the share
  // of the nonzeros in split rows that won. Everything else, unmeasured shapes included, is the
  // plain split hop; HGD_SPMM_BLOCKS_SPLIT forces a block count anywhere.
  const double table = static_cast<double>(n_src_rows) * (d < 128 ? d : 128) * 4.0;
  if (table < 2.56e9 || table >= 5.12e9) return 0;
  const double share = static_cast<double>(n_chunks) * chunk / static_cast<double>(nnz);
  return share <= 0.2862 ? 4 : 0;
}

extern "C" size_t hgd_spmm_col_blocks_ordered_workspace_size(int64_t n_rows, int32_t n_blocks) {
  if (n_rows <= 0 || n_rows >= 0x7fffffffLL || n_blocks <= 0 || n_blocks > 64) return 0;
  return hgd::block_order_ws(n_rows, n_blocks).total;
}

extern "C" hgd_status hgd_spmm_col_blocks_ordered(const int64_t* rowptr, const int32_t* col,
                                                  int64_t n_rows, int64_t n_cols,
                                                  int32_t n_blocks, int64_t* blk_start,
                                                  int32_t* blk_col, int32_t* blk_perm,
                                                  int32_t* blk_out_row, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
  using namespace hgd;
  clear_error();
  constexpr const char* fn = "hgd_spmm_col_blocks_ordered";
  HGD_REQUIRE(n_rows >= 0 && n_cols >= 0, "%s: negative sizes", fn);
  HGD_REQUIRE(n_blocks >= 1 && n_blocks <= 64, "%s: blocks must be 1..64", fn);
  HGD_REQUIRE(n_rows < 0x7fffffffLL, "%s: n_rows >= 2^31 - 1", fn);
  HGD_REQUIRE(n_cols < 0x7fffffffLL, "%s: n_cols >= 2^31 - 1", fn);
  if (n_rows == 0) return HGD_OK;
  HGD_REQUIRE(rowptr && blk_start && blk_out_row, "%s: null rowptr / blk_start / blk_out_row", fn);
  const BlockOrderWs w = block_order_ws(n_rows, n_blocks);
  if (w.total == 0 || !workspace || workspace_bytes < w.total)
    return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < %zu", fn, workspace_bytes, w.total);
  const int64_t n = static_cast<int64_t>(n_blocks) * n_rows;
  const int64_t row_grid = (n_rows + 255) / 256;
  constexpr int kRowsPerBlock = kBlock / kOrdG;
  const int64_t key_grid = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  int64_t* cnt = reinterpret_cast<int64_t*>(ws + w.cnt);      // then the permuted lengths
  int64_t* start = reinterpret_cast<int64_t*>(ws + w.start);  // then the scatter's destinations
  int32_t* keys = reinterpret_cast<int32_t*>(ws + w.keys);
  int32_t* keys_s = reinterpret_cast<int32_t*>(ws + w.keys_s);
  size_t tail_bytes = workspace_bytes - w.tail;
  // the natural block-major copy (hgd_spmm_col_blocks' three steps), into blk_col itself: the
  // keys below are read from it, and the second scatter overwrites it
  hipLaunchKernelGGL(col_block_count_kernel, dim3(row_grid), dim3(256), 0, st, rowptr, col, n_rows,
                     n_cols, n_blocks, cnt);
  hgd_status s = check_launch(fn, "count");
  if (s != HGD_OK) return s;
  HGD_HIP(hipcub::DeviceScan::ExclusiveSum(ws + w.tail, tail_bytes, cnt, start, n + 1, st));
  hipLaunchKernelGGL(col_block_scatter_kernel, dim3(row_grid), dim3(256), 0, st, rowptr, col,
                     n_rows, n_cols, n_blocks, start, blk_col, static_cast<int32_t*>(nullptr));
  s = check_launch(fn, "scatter");
  if (s != HGD_OK) return s;
  // hgd_spmm_row_order's pattern over each block's own CSR (start + k·n_rows, blk_col): keys and
  // stable sort (an empty piece has the key n_cols and sorts last); the rest is any order's
  for (int32_t k = 0; k < n_blocks; ++k) {
    const int64_t off = static_cast<int64_t>(k) * n_rows;
    hipLaunchKernelGGL(row_min_key_kernel, dim3(key_grid), dim3(kBlock), 0, st, start + off,
                       blk_col, n_rows, static_cast<int32_t>(n_cols), keys);
    s = check_launch(fn, "keys");
    if (s != HGD_OK) return s;
    s = hgd_sort_perm(keys, n_rows, n_cols + 1, keys_s, blk_out_row + off, ws + w.tail, tail_bytes,
                      stream);
    if (s != HGD_OK) return s;
  }
  return block_order_tail(fn, rowptr, col, n_rows, n_cols, n_blocks, blk_start, blk_col, blk_perm,
                          blk_out_row, cnt, start, ws + w.tail, tail_bytes, st);
}

extern "C" size_t hgd_spmm_col_blocks_ordered_from_workspace_size(int64_t n_rows,
                                                                  int32_t n_blocks) {
  if (n_rows <= 0 || n_rows >= 0x7fffffffLL || n_blocks <= 0 || n_blocks > 64) return 0;
  const size_t own = hgd::block_order_ws(n_rows, n_blocks).total;
  const size_t check = hgd::order_check_ws(static_cast<int64_t>(n_blocks) * n_rows);
  return own && check ? own + check : 0;
}

extern "C" hgd_status hgd_spmm_col_blocks_ordered_from(const int32_t* blk_order,
                                                       const int64_t* rowptr, const int32_t* col,
                                                       int64_t n_rows, int64_t n_cols,
                                                       int32_t n_blocks, int64_t* blk_start,
                                                       int32_t* blk_col, int32_t* blk_perm,
                                                       void* workspace, size_t workspace_bytes,
                                                       void* stream) {
  using namespace hgd;
  clear_error();
  constexpr const char* fn = "hgd_spmm_col_blocks_ordered_from";
  HGD_REQUIRE(n_rows >= 0 && n_cols >= 0, "%s: negative sizes", fn);
  HGD_REQUIRE(n_blocks >= 1 && n_blocks <= 64, "%s: blocks must be 1..64", fn);
  HGD_REQUIRE(n_rows < 0x7fffffffLL, "%s: n_rows >= 2^31 - 1", fn);
  HGD_REQUIRE(n_cols < 0x7fffffffLL, "%s: n_cols >= 2^31 - 1", fn);
  if (n_rows == 0) return HGD_OK;
  HGD_REQUIRE(rowptr && blk_start && blk_order, "%s: null rowptr / blk_start / blk_order", fn);
  const BlockOrderWs w = block_order_ws(n_rows, n_blocks);
  const size_t need = hgd_spmm_col_blocks_ordered_from_workspace_size(n_rows, n_blocks);
  if (need == 0 || !workspace || workspace_bytes < need)
    return fail(HGD_ERR_WORKSPACE, "%s: workspace %zu < %zu", fn, workspace_bytes, need);
  const int64_t n = static_cast<int64_t>(n_blocks) * n_rows;
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  int64_t* cnt = reinterpret_cast<int64_t*>(ws + w.cnt);
  int64_t* start = reinterpret_cast<int64_t*>(ws + w.start);
  // (the flags where the counts go next; the check's own behind the builder's workspace)
  hgd_status s = check_order(fn, blk_order, n_rows, n, reinterpret_cast<int32_t*>(cnt),
                             ws + w.total, need - w.total, st);
  if (s != HGD_OK) return s;
  // the natural block-major starts (hgd_spmm_col_blocks' count and scan)
  hipLaunchKernelGGL(col_block_count_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, st, rowptr,
                     col, n_rows, n_cols, n_blocks, cnt);
  s = check_launch(fn, "count");
  if (s != HGD_OK) return s;
  size_t tail_bytes = w.total - w.tail;
  HGD_HIP(hipcub::DeviceScan::ExclusiveSum(ws + w.tail, tail_bytes, cnt, start, n + 1, st));
  return block_order_tail(fn, rowptr, col, n_rows, n_cols, n_blocks, blk_start, blk_col, blk_perm,
                          blk_order, cnt, start, ws + w.tail, tail_bytes, st);
}

extern "C" hgd_status hgd_spmm_blocked_ordered(const int64_t* blk_start, const int32_t* blk_col,
                                               const float* blk_val, const float* blk_row_scale,
                                               const int32_t* blk_out_row, int64_t n_rows,
                                               int64_t n_src_rows, const float* X, int64_t ldx,
                                               float* Y, int64_t ldy, int32_t d, int32_t epilogue,
                                               float slope, int32_t n_blocks, void* stream) {
  hgd::clear_error();
  hgd::SpmmRequest r{"hgd_spmm_blocked_ordered", nullptr, blk_col, blk_val, blk_row_scale, n_rows,
                     n_src_rows, 0, n_rows, X, ldx, Y, ldy, d, epilogue, slope};
  r.blocked = true;
  r.blk_start = blk_start;
  r.n_blk = n_blocks;
  r.ordered = true;
  r.out_row = blk_out_row;
  r.stream = stream;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" int32_t hgd_spmm_packed_for(int64_t n_src_rows, int32_t n_blocks, int64_t n_dict,
                                       int32_t idx_bits) {
  if (n_src_rows <= 0 || n_blocks < 2) return 0;  // (one block is not a blocked hop)
  if (!hgd::packed_fits(n_src_rows, n_blocks, n_dict, idx_bits)) return 0;
  // packing changes no sum and takes 4 of the 8 streamed bytes per nonzero away, which pays where
  // the hop's time follows the bytes that leave L2: where the size rules run it block-ordered.
  // The smallest slice hgd_spmm_block_order_for orders is 32 MiB of 512-byte rows (its widest
  // pass, 128 columns); below that many source rows per block the blocks were forced, nothing
  // was measured and the rule is off (HGD_SPMM_PACKED=1 packs wherever it fits)
  return n_src_rows / n_blocks >= 65536 ? 1 : 0;
}

extern "C" int32_t hgd_spmm_packed_fits(int64_t n_src_rows, int32_t n_blocks, int64_t n_dict,
                                        int32_t idx_bits) {
  return hgd::packed_fits(n_src_rows, n_blocks, n_dict, idx_bits) ? 1 : 0;
}

extern "C" hgd_status hgd_spmm_pack_entries(const int64_t* blk_start, const int32_t* blk_col,
                                            const int32_t* src_code, int64_t n_rows,
                                            int64_t n_src_rows, int64_t nnz, int32_t n_blocks,
                                            int32_t n_dict, int32_t idx_bits, uint32_t* ent,
                                            void* stream) {
  using namespace hgd;
  clear_error();
  constexpr const char* fn = "hgd_spmm_pack_entries";
  HGD_REQUIRE(n_rows >= 0 && n_src_rows >= 0 && nnz >= 0, "%s: negative sizes", fn);
  HGD_REQUIRE(n_blocks >= 1 && n_blocks <= 64, "%s: blocks must be 1..64", fn);
  HGD_REQUIRE(n_src_rows < (int64_t(1) << 31), "%s: n_src_rows >= 2^31", fn);
  HGD_REQUIRE(idx_bits >= 1 && idx_bits <= 31, "%s: idx_bits must be 1..31 (got %d)", fn, idx_bits);
  HGD_REQUIRE(n_dict >= 1, "%s: n_dict must be >= 1 (got %d)", fn, n_dict);
  if (!packed_fits(n_src_rows, n_blocks, n_dict, idx_bits))
    return fail(HGD_ERR_UNSUPPORTED,
                "%s: %d blocks of %lld source rows and %d weights do not fit %d + %d bits (at most "
                "%d weights)", fn, n_blocks, (long long)n_src_rows, n_dict, idx_bits, 32 - idx_bits,
                HGD_SPMM_PACKED_MAX_DICT);
  if (nnz == 0) return HGD_OK;
  HGD_REQUIRE(blk_start && blk_col && src_code && ent,
              "%s: null blk_start / blk_col / src_code / ent", fn);
  const int64_t grid = (nnz + kBlock - 1) / kBlock;
  HGD_REQUIRE(grid <= 0x7fffffffLL, "%s: too many nonzeros", fn);
  hipLaunchKernelGGL(pack_entries_kernel, dim3(grid), dim3(kBlock), 0, as_stream(stream),
                     blk_start, blk_col, src_code, n_rows, n_src_rows, nnz, n_blocks, idx_bits,
                     ent);
  return check_launch(fn, "kernel");
}

extern "C" hgd_status hgd_spmm_blocked_packed(const int64_t* blk_start, const uint32_t* ent,
                                              const float* dict, int32_t n_dict, int32_t idx_bits,
                                              const float* blk_row_scale,
                                              const int32_t* blk_out_row, int64_t n_rows,
                                              int64_t n_src_rows, const float* X, int64_t ldx,
                                              float* Y, int64_t ldy, int32_t d, int32_t epilogue,
                                              float slope, int32_t n_blocks, void* stream) {
  hgd::clear_error();
  hgd::SpmmRequest r{"hgd_spmm_blocked_packed", nullptr, reinterpret_cast<const int32_t*>(ent),
                     nullptr, blk_row_scale, n_rows, n_src_rows, 0, n_rows, X, ldx, Y, ldy, d,
                     epilogue, slope};
  r.blocked = true;
  r.blk_start = blk_start;
  r.n_blk = n_blocks;
  r.ordered = true;
  r.out_row = blk_out_row;
  r.packed = true;
  r.dict = dict;
  r.n_dict = n_dict;
  r.idx_bits = idx_bits;
  r.stream = stream;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" hgd_status hgd_spmm_fused(const int64_t* rowptr, const int32_t* col, const float* val,
                                     const float* row_scale, int64_t n_rows, int64_t n_src_rows,
                                     int64_t row_begin, int64_t row_end, const float* X,
                                     int64_t ldx, float* Y, int64_t ldy, int32_t d,
                                     const hgd_row_epilogue* epi, const hgd_split_plan* plan,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(epi != nullptr, "hgd_spmm_fused: null epilogue descriptor");
  hgd::SpmmRequest r{"hgd_spmm_fused", rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                     row_end, X, ldx, Y, ldy, d, epi->act, epi->slope, plan, workspace,
                     workspace_bytes, stream};
  r.ex = epi;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" hgd_status hgd_spmm_masked(const int64_t* rowptr, const int32_t* col, const float* val,
                                      const uint8_t* mask, float keep, const float* row_scale,
                                      int64_t n_rows, int64_t n_src_rows, int64_t row_begin,
                                      int64_t row_end, const float* X, int64_t ldx, float* Y,
                                      int64_t ldy, int32_t d, int32_t epilogue, float slope,
                                      const hgd_split_plan* plan, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  hgd::SpmmRequest r{"hgd_spmm_masked", rowptr, col, val, row_scale, n_rows, n_src_rows, row_begin,
                     row_end, X, ldx, Y, ldy, d, epilogue, slope, plan, workspace, workspace_bytes,
                     stream};
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" hgd_status hgd_spmm_masked_fused(const int64_t* rowptr, const int32_t* col,
                                            const float* val, const uint8_t* mask, float keep,
                                            const float* row_scale, int64_t n_rows,
                                            int64_t n_src_rows, int64_t row_begin,
                                            int64_t row_end, const float* X, int64_t ldx,
                                            float* Y, int64_t ldy, int32_t d,
                                            const hgd_row_epilogue* epi,
                                            const hgd_split_plan* plan, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(epi != nullptr, "hgd_spmm_masked_fused: null epilogue descriptor");
  hgd::SpmmRequest r{"hgd_spmm_masked_fused", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, epi->act, epi->slope, plan, workspace,
                     workspace_bytes, stream};
  r.ex = epi;
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  return hgd::spmm_launch<float, float>(r);
}

// The ordered twins of the three entry points above (hgd_spmm_ordered's contract: rowptr / col /
// val / row_scale the ordered copies, out_row the order, every row): mask is in the ordered entry
// order, everything epi points to stays indexed by Y row.
extern "C" hgd_status hgd_spmm_fused_ordered(const int64_t* rowptr, const int32_t* col,
                                             const float* val, const float* row_scale,
                                             int64_t n_rows, int64_t n_src_rows,
                                             int64_t row_begin, int64_t row_end, const float* X,
                                             int64_t ldx, float* Y, int64_t ldy, int32_t d,
                                             const hgd_row_epilogue* epi,
                                             const hgd_split_plan* plan, void* workspace,
                                             size_t workspace_bytes, const int32_t* out_row,
                                             void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(epi != nullptr, "hgd_spmm_fused_ordered: null epilogue descriptor");
  hgd::SpmmRequest r{"hgd_spmm_fused_ordered", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, epi->act, epi->slope, plan, workspace,
                     workspace_bytes, stream};
  r.ex = epi;
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" hgd_status hgd_spmm_masked_ordered(const int64_t* rowptr, const int32_t* col,
                                              const float* val, const uint8_t* mask, float keep,
                                              const float* row_scale, int64_t n_rows,
                                              int64_t n_src_rows, int64_t row_begin,
                                              int64_t row_end, const float* X, int64_t ldx,
                                              float* Y, int64_t ldy, int32_t d, int32_t epilogue,
                                              float slope, const hgd_split_plan* plan,
                                              void* workspace, size_t workspace_bytes,
                                              const int32_t* out_row, void* stream) {
  hgd::clear_error();
  hgd::SpmmRequest r{"hgd_spmm_masked_ordered", rowptr, col, val, row_scale, n_rows, n_src_rows,
                     row_begin, row_end, X, ldx, Y, ldy, d, epilogue, slope, plan, workspace,
                     workspace_bytes, stream};
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_launch<float, float>(r);
}

extern "C" hgd_status hgd_spmm_masked_fused_ordered(const int64_t* rowptr, const int32_t* col,
                                                    const float* val, const uint8_t* mask,
                                                    float keep, const float* row_scale,
                                                    int64_t n_rows, int64_t n_src_rows,
                                                    int64_t row_begin, int64_t row_end,
                                                    const float* X, int64_t ldx, float* Y,
                                                    int64_t ldy, int32_t d,
                                                    const hgd_row_epilogue* epi,
                                                    const hgd_split_plan* plan, void* workspace,
                                                    size_t workspace_bytes,
                                                    const int32_t* out_row, void* stream) {
  hgd::clear_error();
  HGD_REQUIRE(epi != nullptr, "hgd_spmm_masked_fused_ordered: null epilogue descriptor");
  hgd::SpmmRequest r{"hgd_spmm_masked_fused_ordered", rowptr, col, val, row_scale, n_rows,
                     n_src_rows, row_begin, row_end, X, ldx, Y, ldy, d, epi->act, epi->slope,
                     plan, workspace, workspace_bytes, stream};
  r.ex = epi;
  r.masked = true;
  r.mask = mask;
  r.keep = keep;
  r.ordered = true;
  r.out_row = out_row;
  return hgd::spmm_launch<float, float>(r);
}
