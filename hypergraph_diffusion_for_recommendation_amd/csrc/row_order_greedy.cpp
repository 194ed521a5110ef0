// Greedy shared-column row orders for the ordered hops (hgd_row_order_greedy,
// hgd_col_block_order_greedy): the next row walked is one that shares the most columns with what
// the XCD's L2 still holds. Plain host C++ over host pointers — no HIP call, no device memory — so
// it builds and runs without a GPU.
//
// The model the order is built for (scripts/model_l2_order.py): workgroups of rows_per_wg rows are
// dealt round-robin to n_xcd XCDs, an XCD walks its workgroups in order and a row's gathers in
// edge order, and a gather hits when the same XCD fetched that source row within its last
// `window` gathers. So every XCD gets a contiguous natural range of the rows (a part), the greedy
// walk runs inside the part (cut evenly into chunks_per_xcd chunks to bound the build), and the
// parts are interleaved in whole workgroups so that XCD x walks part x from its start to its end.
//
// One chunk: a FIFO of the last `window` gathered columns with a count per column; cnt[row] =
// the distinct counted columns of an unplaced row now in the FIFO, kept up to date through the
// chunk's own transposed lists whenever a column's count goes 0 -> 1 or 1 -> 0; the rows with
// cnt >= 1 in buckets by cnt (intrusive doubly linked lists, a move is O(1)). The next row is the
// shortest of the few most recently moved rows of the highest bucket; without one, the chunk's
// next unplaced row in min-column order. A column of more than col_cap entries in the chunk sits
// in the FIFO but moves no row: it bounds the work at 2·nnz·min(degree, col_cap) list moves.
//
// The result depends on the arguments only: a chunk is walked by one thread and writes its own
// range of the output, whatever the thread count.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <new>
#include <thread>
#include <vector>

#include "../../include/hgd.h"

namespace hgd {

// (structure.hip's; a stand-alone program brings its own)
extern thread_local char g_last_error[512];

namespace {

hgd_status greedy_fail(hgd_status st, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
  return st;
}

// How many rows of the highest bucket the pick looks at (modelled at 50,000 × 5,000 × 500,000,
// window 81, 8 parts: 20.3 % of the gathers hit with 1, 21.3 % with 4, 21.6 % with 8, 21.8 % with
// 64).
constexpr int kPickScan = 8;

// The pieces the walk runs over: row r's entries are [pb[r·stride], pe[r·stride]) of col, all in
// the column range [c_lo, c_hi). The whole structure: pb = rowptr, pe = rowptr + 1, stride 1.
struct Pieces {
  const int64_t* pb;
  const int64_t* pe;
  int64_t stride;
  const int32_t* col;
  int64_t c_lo, c_hi;
  int64_t begin(int64_t r) const { return pb[r * stride]; }
  int64_t end(int64_t r) const { return pe[r * stride]; }
};

// Walks the m non-empty rows `rows` (ascending) and writes them to out[0, m) in greedy order.
// False when a column lies outside the range.
bool greedy_chunk(const Pieces& p, const int32_t* rows, int64_t m, int64_t window, int64_t col_cap,
                  int32_t* out) {
  if (m == 0) return true;
  const int64_t nc = p.c_hi - p.c_lo;
  // the chunk's transposed lists (local row ids, ascending per column), the rows' min-column keys
  // and the longest piece (the highest bucket there can be)
  std::vector<int64_t> tptr(static_cast<size_t>(nc) + 1, 0);
  std::vector<int32_t> key(static_cast<size_t>(m));
  int64_t max_len = 0;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t b = p.begin(rows[i]), e = p.end(rows[i]);
    int64_t lo = nc;
    for (int64_t j = b; j < e; ++j) {
      const int64_t c = static_cast<int64_t>(p.col[j]) - p.c_lo;
      if (c < 0 || c >= nc) return false;
      ++tptr[static_cast<size_t>(c) + 1];
      lo = std::min(lo, c);
    }
    key[static_cast<size_t>(i)] = static_cast<int32_t>(lo);
    max_len = std::max(max_len, e - b);
  }
  for (int64_t c = 0; c < nc; ++c) tptr[static_cast<size_t>(c) + 1] += tptr[static_cast<size_t>(c)];
  std::vector<int32_t> tl(static_cast<size_t>(tptr[static_cast<size_t>(nc)]));
  {
    std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t j = p.begin(rows[i]), e = p.end(rows[i]); j < e; ++j)
        tl[static_cast<size_t>(fill[static_cast<size_t>(p.col[j] - p.c_lo)]++)] =
            static_cast<int32_t>(i);
  }
  // the fall-back order: ascending smallest column, ties in natural order
  std::vector<int32_t> by_min(static_cast<size_t>(m));
  for (int64_t i = 0; i < m; ++i) by_min[static_cast<size_t>(i)] = static_cast<int32_t>(i);
  std::stable_sort(by_min.begin(), by_min.end(), [&](int32_t a, int32_t b) {
    return key[static_cast<size_t>(a)] < key[static_cast<size_t>(b)];
  });
  key = std::vector<int32_t>();

  std::vector<int32_t> cnt(static_cast<size_t>(m), 0);  // -1: placed
  std::vector<int32_t> nxt(static_cast<size_t>(m), -1), prv(static_cast<size_t>(m), -1);
  std::vector<int32_t> head(static_cast<size_t>(max_len) + 1, -1);  // bucket 0 is not a list
  std::vector<int32_t> in_fifo(static_cast<size_t>(nc), 0);
  // (a window the chunk's gathers never fill is one of exactly that many)
  window = std::min<int64_t>(window, std::max<int64_t>(1, static_cast<int64_t>(tl.size())));
  std::vector<int32_t> fifo(static_cast<size_t>(window));
  int64_t fifo_at = 0, fifo_n = 0;  // the oldest entry and how many there are
  int32_t top = 0;                  // no bucket above it is occupied
  int32_t* const cn = cnt.data();
  int32_t* const nx = nxt.data();
  int32_t* const pv = prv.data();
  int32_t* const hd = head.data();

  auto unlink = [&](int32_t t, int32_t b) {
    const int32_t n = nx[t], q = pv[t];
    if (q >= 0) nx[q] = n; else hd[b] = n;
    if (n >= 0) pv[n] = q;
  };
  auto link = [&](int32_t t, int32_t b) {
    const int32_t h = hd[b];
    nx[t] = h;
    pv[t] = -1;
    if (h >= 0) pv[h] = t;
    hd[b] = t;
  };
  auto counted = [&](int64_t c) {
    return tptr[static_cast<size_t>(c) + 1] - tptr[static_cast<size_t>(c)] <= col_cap;
  };
  auto column_in = [&](int64_t c) {
    const int64_t e = tptr[static_cast<size_t>(c) + 1];
    for (int64_t j = tptr[static_cast<size_t>(c)]; j < e; ++j) {
      const int32_t t = tl[static_cast<size_t>(j)];
      const int32_t b = cn[t];
      if (b < 0) continue;
      if (b >= 1) unlink(t, b);
      cn[t] = b + 1;
      link(t, b + 1);
      if (b + 1 > top) top = b + 1;
    }
  };
  auto column_out = [&](int64_t c) {
    const int64_t e = tptr[static_cast<size_t>(c) + 1];
    for (int64_t j = tptr[static_cast<size_t>(c)]; j < e; ++j) {
      const int32_t t = tl[static_cast<size_t>(j)];
      const int32_t b = cn[t];
      if (b < 1) continue;  // placed (an unplaced row that holds a counted column has b >= 1)
      unlink(t, b);
      cn[t] = b - 1;
      if (b > 1) link(t, b - 1);
    }
  };

  int64_t fall = 0;
  for (int64_t k = 0; k < m; ++k) {
    while (top >= 1 && hd[top] < 0) --top;
    int32_t i;
    if (top >= 1) {
      // of the kPickScan most recently moved rows of the bucket the shortest (the first of equals):
      // it shares as many columns and pushes the fewest others out of the window
      i = hd[top];
      int64_t best = p.end(rows[i]) - p.begin(rows[i]);
      int32_t t = nx[i];
      for (int q = 1; q < kPickScan && t >= 0; ++q, t = nx[t]) {
        const int64_t len = p.end(rows[t]) - p.begin(rows[t]);
        if (len < best) {
          best = len;
          i = t;
        }
      }
      unlink(i, top);
    } else {
      while (cn[by_min[static_cast<size_t>(fall)]] < 0) ++fall;
      i = by_min[static_cast<size_t>(fall)];
    }
    cn[i] = -1;
    out[k] = rows[i];
    for (int64_t j = p.begin(rows[i]), e = p.end(rows[i]); j < e; ++j) {
      const int64_t c = static_cast<int64_t>(p.col[j]) - p.c_lo;
      int64_t slot;
      if (fifo_n == window) {  // the oldest gather leaves
        const int64_t o = fifo[static_cast<size_t>(fifo_at)];
        if (--in_fifo[static_cast<size_t>(o)] == 0 && counted(o)) column_out(o);
        slot = fifo_at;
        fifo_at = fifo_at + 1 == window ? 0 : fifo_at + 1;
      } else {
        slot = fifo_at + fifo_n;
        if (slot >= window) slot -= window;
        ++fifo_n;
      }
      fifo[static_cast<size_t>(slot)] = static_cast<int32_t>(c);
      if (in_fifo[static_cast<size_t>(c)]++ == 0 && counted(c)) column_in(c);
    }
  }
  return true;
}

int pick_threads(int32_t threads, int64_t n_tasks) {
  int64_t t = threads;
  if (t <= 0) {
    t = 8;
    if (const char* e = std::getenv("OMP_NUM_THREADS")) {
      const long v = std::strtol(e, nullptr, 10);
      if (v >= 1) t = v;
    }
  }
  t = std::min<int64_t>(t, n_tasks);
  return static_cast<int>(std::max<int64_t>(t, 1));
}

struct Task {
  Pieces p;
  const int32_t* rows;
  int64_t m;
  int32_t* out;
};

// Runs the tasks on up to `threads` threads (each task by one thread, into its own range) and
// turns what went wrong into a status: a column out of range, or no memory for a chunk's tables.
// No exception leaves it: a thread that cannot be started is done without (the threads that did
// start, and this one, take its tasks: the order does not depend on their number).
hgd_status run_tasks(const char* fn, const std::vector<Task>& tasks, int64_t window,
                     int64_t col_cap, int32_t threads) {
  std::atomic<size_t> next{0};
  std::atomic<int> bad_column{0}, no_memory{0};
  auto work = [&]() noexcept {
    for (size_t i = next.fetch_add(1); i < tasks.size(); i = next.fetch_add(1)) {
      const Task& t = tasks[i];
      try {
        if (!greedy_chunk(t.p, t.rows, t.m, window, col_cap, t.out)) bad_column.store(1);
      } catch (const std::exception&) {  // (bad_alloc, length_error: a table that cannot be made)
        no_memory.store(1);
      }
    }
  };
  const int n = pick_threads(threads, static_cast<int64_t>(tasks.size()));
  std::vector<std::thread> th;
  try {
    th.reserve(static_cast<size_t>(n));
    for (int i = 1; i < n; ++i) th.emplace_back(work);
  } catch (const std::exception&) {  // (system_error: no more threads to be had)
  }
  work();
  for (auto& t : th) t.join();
  if (bad_column.load())
    return greedy_fail(HGD_ERR_INVALID_ARG, "%s: a column outside [0, n_cols)", fn);
  if (no_memory.load()) return greedy_fail(HGD_ERR_WORKSPACE, "%s: out of host memory", fn);
  return HGD_OK;
}

// The parts and chunks of one walk over the non-empty rows ne[0, m): part x is the natural range
// that XCD x's workgroups hold (workgroup w = positions [w·R, (w+1)·R) goes to XCD w mod X; only
// the last workgroup is short), cut evenly into C chunks; the tasks write the parts one after the
// other into seq[0, m).
void add_tasks(const Pieces& p, const int32_t* ne, int64_t m, int64_t R, int64_t X, int64_t C,
               int32_t* seq, std::vector<Task>& tasks, std::vector<int64_t>& part_off) {
  const int64_t n_wg = (m + R - 1) / R;
  part_off.assign(static_cast<size_t>(X) + 1, 0);
  for (int64_t x = 0; x < X; ++x) {
    const int64_t wgs = n_wg / X + (x < n_wg % X ? 1 : 0);
    int64_t size = wgs * R;
    if (n_wg > 0 && (n_wg - 1) % X == x) size -= n_wg * R - m;  // the short last workgroup
    part_off[static_cast<size_t>(x) + 1] = part_off[static_cast<size_t>(x)] + size;
    for (int64_t c = 0; c < C; ++c) {
      const int64_t b = part_off[static_cast<size_t>(x)] + size * c / C;
      const int64_t e = part_off[static_cast<size_t>(x)] + size * (c + 1) / C;
      if (e > b) tasks.push_back(Task{p, ne + b, e - b, seq + b});
    }
  }
}

// Position (X·s + x)·R + j takes element s·R + j of part x.
void place_parts(const int32_t* seq, const std::vector<int64_t>& part_off, int64_t R, int64_t X,
                 int32_t* order) {
  for (int64_t x = 0; x < X; ++x) {
    const int64_t off = part_off[static_cast<size_t>(x)];
    const int64_t size = part_off[static_cast<size_t>(x) + 1] - off;
    for (int64_t t = 0; t < size; ++t) order[(X * (t / R) + x) * R + t % R] = seq[off + t];
  }
}

hgd_status check_common(const char* fn, const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                        int64_t n_cols, int64_t window, int32_t col_cap, int32_t rows_per_wg,
                        int32_t n_xcd, int32_t chunks_per_xcd, int32_t threads, const void* out) {
  if (n_rows < 0 || n_cols < 0) return greedy_fail(HGD_ERR_INVALID_ARG, "%s: negative sizes", fn);
  if (n_rows >= 0x7fffffffLL || n_cols >= 0x7fffffffLL)
    return greedy_fail(HGD_ERR_INVALID_ARG, "%s: n_rows / n_cols >= 2^31 - 1", fn);
  if (window < 1 || window > 0x7fffffffLL)
    return greedy_fail(HGD_ERR_INVALID_ARG, "%s: window must be 1..2^31-1 (got %lld)", fn,
                       static_cast<long long>(window));
  if (col_cap < 1) return greedy_fail(HGD_ERR_INVALID_ARG, "%s: col_cap must be >= 1", fn);
  if (rows_per_wg < 1 || n_xcd < 1 || chunks_per_xcd < 1)
    return greedy_fail(HGD_ERR_INVALID_ARG,
                       "%s: rows_per_wg, n_xcd and chunks_per_xcd must be >= 1", fn);
  if (threads < 0) return greedy_fail(HGD_ERR_INVALID_ARG, "%s: threads must be >= 0", fn);
  if (n_rows > 0 && (!rowptr || !out))
    return greedy_fail(HGD_ERR_INVALID_ARG, "%s: null rowptr / output", fn);
  if (n_rows > 0) {
    if (rowptr[0] < 0) return greedy_fail(HGD_ERR_INVALID_ARG, "%s: rowptr[0] < 0", fn);
    for (int64_t r = 0; r < n_rows; ++r)
      if (rowptr[r + 1] < rowptr[r])
        return greedy_fail(HGD_ERR_INVALID_ARG, "%s: rowptr descends at row %lld", fn,
                           static_cast<long long>(r));
    if (rowptr[n_rows] > rowptr[0] && !col)
      return greedy_fail(HGD_ERR_INVALID_ARG, "%s: null col", fn);
  }
  return HGD_OK;
}

}  // namespace
}  // namespace hgd

extern "C" hgd_status hgd_row_order_greedy(const int64_t* rowptr, const int32_t* col,
                                           int64_t n_rows, int64_t n_cols, int64_t window,
                                           int32_t col_cap, int32_t rows_per_wg, int32_t n_xcd,
                                           int32_t chunks_per_xcd, int32_t threads,
                                           int32_t* order_out) {
  using namespace hgd;
  constexpr const char* fn = "hgd_row_order_greedy";
  g_last_error[0] = '\0';
  hgd_status s = check_common(fn, rowptr, col, n_rows, n_cols, window, col_cap, rows_per_wg, n_xcd,
                              chunks_per_xcd, threads, order_out);
  if (s != HGD_OK || n_rows == 0) return s;
  try {
    std::vector<int32_t> ne, seq;
    int64_t n_empty = 0;
    for (int64_t r = 0; r < n_rows; ++r)
      if (rowptr[r + 1] > rowptr[r]) ne.push_back(static_cast<int32_t>(r));
    const int64_t m = static_cast<int64_t>(ne.size());
    for (int64_t r = 0; r < n_rows; ++r)  // empty rows last, in natural order
      if (rowptr[r + 1] == rowptr[r]) order_out[m + n_empty++] = static_cast<int32_t>(r);
    seq.resize(ne.size());
    const Pieces p{rowptr, rowptr + 1, 1, col, 0, n_cols};
    std::vector<Task> tasks;
    std::vector<int64_t> part_off;
    add_tasks(p, ne.data(), m, rows_per_wg, n_xcd, chunks_per_xcd, seq.data(), tasks, part_off);
    s = run_tasks(fn, tasks, window, col_cap, threads);
    if (s != HGD_OK) return s;
    place_parts(seq.data(), part_off, rows_per_wg, n_xcd, order_out);
  } catch (const std::exception&) {
    return greedy_fail(HGD_ERR_WORKSPACE, "%s: out of host memory", fn);
  }
  return HGD_OK;
}

extern "C" hgd_status hgd_col_block_order_greedy(const int64_t* rowptr, const int32_t* col,
                                                 int64_t n_rows, int64_t n_cols, int32_t n_blocks,
                                                 int64_t window, int32_t col_cap,
                                                 int32_t rows_per_wg, int32_t n_xcd,
                                                 int32_t chunks_per_xcd, int32_t threads,
                                                 int32_t* blk_order_out) {
  using namespace hgd;
  constexpr const char* fn = "hgd_col_block_order_greedy";
  g_last_error[0] = '\0';
  if (n_blocks < 1 || n_blocks > 64)
    return greedy_fail(HGD_ERR_INVALID_ARG, "%s: blocks must be 1..64", fn);
  hgd_status s = check_common(fn, rowptr, col, n_rows, n_cols, window, col_cap, rows_per_wg, n_xcd,
                              chunks_per_xcd, threads, blk_order_out);
  if (s != HGD_OK || n_rows == 0) return s;
  try {
    const int64_t P = n_blocks;
    // cut[r·(P+1) + k] = the first entry of row r in block k (its columns ascend), closed by the
    // row's end: block k's piece of row r is [cut[.. + k], cut[.. + k + 1])
    std::vector<int64_t> cut(static_cast<size_t>(n_rows) * static_cast<size_t>(P + 1));
    for (int64_t r = 0; r < n_rows; ++r) {
      int64_t* c = cut.data() + r * (P + 1);
      int64_t k = 0, prev = -1;
      c[0] = rowptr[r];
      for (int64_t j = rowptr[r]; j < rowptr[r + 1]; ++j) {
        const int64_t v = col[j];
        if (v < prev || v < 0 || v >= n_cols)
          return greedy_fail(HGD_ERR_INVALID_ARG,
                             "%s: row %lld's columns do not ascend inside [0, n_cols)", fn,
                             static_cast<long long>(r));
        prev = v;
        while (k + 1 < P && v >= n_cols * (k + 1) / P) c[++k] = j;
      }
      while (k < P) c[++k] = rowptr[r + 1];
    }
    std::vector<int32_t> ne(static_cast<size_t>(n_rows) * static_cast<size_t>(P));
    std::vector<int32_t> seq(ne.size());
    std::vector<int64_t> m(static_cast<size_t>(P), 0);
    std::vector<std::vector<int64_t>> part_off(static_cast<size_t>(P));
    std::vector<Task> tasks;
    for (int64_t k = 0; k < P; ++k) {
      int32_t* nek = ne.data() + k * n_rows;
      int32_t* outk = blk_order_out + k * n_rows;
      int64_t n_empty = 0, mk = 0;
      for (int64_t r = 0; r < n_rows; ++r)
        if (cut[r * (P + 1) + k + 1] > cut[r * (P + 1) + k]) nek[mk++] = static_cast<int32_t>(r);
      for (int64_t r = 0; r < n_rows; ++r)  // rows without a nonzero in the block last
        if (cut[r * (P + 1) + k + 1] == cut[r * (P + 1) + k])
          outk[mk + n_empty++] = static_cast<int32_t>(r);
      m[static_cast<size_t>(k)] = mk;
      const Pieces p{cut.data() + k, cut.data() + k + 1, P + 1, col, n_cols * k / P,
                     n_cols * (k + 1) / P};
      add_tasks(p, nek, mk, rows_per_wg, n_xcd, chunks_per_xcd, seq.data() + k * n_rows, tasks,
                part_off[static_cast<size_t>(k)]);
    }
    s = run_tasks(fn, tasks, window, col_cap, threads);
    if (s != HGD_OK) return s;
    for (int64_t k = 0; k < P; ++k)
      place_parts(seq.data() + k * n_rows, part_off[static_cast<size_t>(k)], rows_per_wg, n_xcd,
                  blk_order_out + k * n_rows);
  } catch (const std::exception&) {
    return greedy_fail(HGD_ERR_WORKSPACE, "%s: out of host memory", fn);
  }
  return HGD_OK;
}
