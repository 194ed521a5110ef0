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
//
// The pooled walk (hgd_row_order_greedy_pooled, hgd_col_block_order_greedy_pooled): the same
// layout, but the XCDs of a group of xcds_per_pool pick their rows from ONE pool, the natural
// range their parts cover together. Every XCD of the group is a walker with its own FIFO and its
// own count per row of the whole pool; in round s walker 0, 1, ... each take their s-th row, a
// higher walker never a row a lower one took in that round. A walker so chooses among
// xcds_per_pool times as many rows as in a part of its own.
//
// It runs in parallel and still depends on the arguments only: the pool's rows are cut evenly
// into K contiguous ranges, each of a logical owner (K is a power of two up to 16, from the
// pool's entries per column alone). An owner holds the transposed lists of its rows and, for
// every walker, their counts (as narrow as the longest row allows) and, per count >= 2, a stack
// of the rows that came to that count, most recent on top. A round:
//   1. every owner proposes, per walker, the kPickScan most recent rows of its highest count,
//      shortest first, then lower row first;
//   2. every thread makes the same reduction over the proposals, walker by walker: the highest
//      count, then the shortest row, then the lowest row that nobody took in this round; without
//      one, the pool's next unplaced row in min-column order. The thread that keeps a walker's
//      FIFO pushes the row's columns through it and lists the columns that went 0 -> 1 and 1 -> 0;
//   3. every owner marks the picked rows placed for all walkers and applies the walkers' column
//      lists, in walker order, to its own rows: a move is one write to a count and, at counts of
//      2 and more, a push on a stack (a row leaves its old entry behind: an entry is good while
//      its row's count is the stack's; stale ones are dropped when they surface).
// Two barriers a round (after 1 and after 2), which spin briefly and then yield. An owner is
// always run by the same thread of the pool's team, and the pools of one call (the groups, the
// source blocks) are dealt to teams of threads by their index. Placed rows are packed out of an
// owner's lists whenever they make a quarter of them.
//
// Departures from the pick rule of one chunk, all modelled (scripts/model_l2_order.py --pool):
// recency is kept per owner, so up to K·kPickScan rows of the highest count are compared and the
// shortest of them wins, not the most recent of the shortest; rows of count 1 keep no list and are
// found through the walker's kRecentCols most recent columns; a column is counted by its entries
// in the pool; and where the window is long a walker takes several rows a round (kRoundShare).
// At 50,000 × 5,000 × 500,000, window 81: 21.6 % of the gathers into users hit with 8 parts walked
// alone, 27.7 % with one pool of 8 walkers; block 0 of 4 into items 6.8 % and 9.1 %.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <limits>
#include <memory>
#include <new>
#include <stdexcept>
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

  // ---------------------------------------------------------------------------------------------
  // The pooled walk
  // ---------------------------------------------------------------------------------------------
  constexpr int kMaxOwners = 16;
  // A walker takes up to kMaxRowsPerRound rows a round, as long as their gathers stay under a
  // 1/kRoundShare of its window: the rows of one round are chosen without seeing each other's
  // columns, which costs hits by the share of the window a round fills (modelled at 500,000 ×
  // 50,000 × 5,000,000, window 819: 29.03 % into users with 1 row a round, 28.93 % with 2 or 2.4 % of
  // the window, 28.72 % with 4) and saves that many barriers and proposals.
  constexpr int64_t kMaxRowsPerRound = 8, kRoundShare = 128;

  // A barrier of a team's threads: a short spin, then the processor is given up on every look (a
  // peer that has been descheduled gets it).
  class TeamBarrier {
   public:
    explicit TeamBarrier(int n) : n_(n) {}
    void wait() {
      if (n_ == 1) return;
      const int g = gen_.load(std::memory_order_acquire);
      if (count_.fetch_add(1, std::memory_order_acq_rel) + 1 == n_) {
        count_.store(0, std::memory_order_relaxed);
        gen_.store(g + 1, std::memory_order_release);
        return;
      }
      for (int spin = 0; gen_.load(std::memory_order_acquire) == g; ++spin)
        if (spin >= 512) std::this_thread::yield();
    }

   private:
    const int n_;
    std::atomic<int> count_{0}, gen_{0};
  };

  // One pool: the m non-empty rows `rows` (ascending), walked by G walkers; walker g takes size[g]
  // rows (they add up to m) and writes them to seq + off[g] in the order it took them.
  struct Pool {
    Pieces p;
    const int32_t* rows;
    int64_t m;
    int32_t* seq;
    std::vector<int64_t> size, off;
    int64_t nnz, max_len;
    int K;  // logical owners
  };

  // What an owner offers a walker, in one cache line (the reduction reads every owner's): pool-local
  // rows, shortest first, then lower first; a length above 65,535 counts as that.
  struct alignas(64) Proposal {
    int32_t cnt, n;
    int32_t row[kPickScan];
    uint16_t len[kPickScan];
  };
  static_assert(sizeof(Proposal) == 64, "a proposal is a cache line");

  // How many of a walker's most recent 0 -> 1 columns an owner looks through for rows of count 1,
  // and how far down a bucket's stack it looks for kPickScan rows that are still there.
  constexpr int kRecentCols = 32;
  constexpr int kStackLook = 64;

  // What the owner of the pool-local rows [lo, lo + n) holds: the transposed lists of its rows and,
  // per walker, their counts (Cnt: as narrow as the longest row allows; its largest value marks a
  // placed row) and, per count b >= 2, a stack of the rows that came to b, the most recent on top.
  // An entry is good while its row's count is still b: a row that moves on leaves its entry behind
  // (a move is one write to the count and at most one push), stale entries are dropped when they
  // surface, and a stack that outgrows twice the owner's rows is swept. Rows of count 1 keep no
  // stack: they are found through the walker's most recent columns.
  template <class Cnt>
  struct Owner {
    static constexpr Cnt kPlaced = std::numeric_limits<Cnt>::max();
    int64_t lo = 0, n = 0;
    std::vector<uint32_t> tptr;  // owner-local ids, ascending per column
    std::vector<int32_t> tl, len;
    std::vector<Cnt> cnt;                      // [G][n]
    std::vector<std::vector<int32_t>> stack;   // [G][max_len + 1]
    std::vector<int32_t> top;                  // [G]: no stack above it holds a good entry
    std::vector<uint8_t> mark;                 // [n], all 0 between sweeps
    int64_t live = 0, gone = 0;                // rows the lists held when last packed; placed since
  };

  template <class Cnt>
  struct PoolState {
    std::vector<Owner<Cnt>> owners;
    std::vector<int32_t> key, by_min, coldeg;  // min column per row; the fall-back order; entries
    std::vector<uint8_t> placed;
    std::vector<int32_t> in_fifo;              // [G][nc]
    std::vector<std::vector<int32_t>> fifo;    // [G][window]
    std::vector<int64_t> fifo_at, fifo_n;
    std::vector<std::vector<uint32_t>> events;  // [G]: column · 2 + (1: 0 -> 1, 0: 1 -> 0)
    std::vector<int32_t> recent;               // [G][kRecentCols]: the last 0 -> 1 columns, a ring
    std::vector<int64_t> recent_n;             // [G]: how many there have been
    std::vector<Proposal> prop;                // [G][K]
    std::atomic<int> bad_column{0}, no_memory{0};
    // no memory in a round: set only between the round's second barrier and the next one's first
    // (fail_apply) or between a round's two barriers (fail_fifo), and read right after the barrier
    // that ends that span, so that every member reads the same and they leave together
    std::atomic<int> fail_apply{0}, fail_fifo{0};
  };

  struct Team {
    explicit Team(int n) : size(n), barrier(n) {}
    int size;
    TeamBarrier barrier;
    void* state = nullptr;  // the PoolState of the pool the team is at, member 0's to make and free
  };

  template <class Cnt>
  bool build_owner(const Pool& pl, int G, Owner<Cnt>& o, int32_t* key) {
    const Pieces& p = pl.p;
    const int64_t nc = p.c_hi - p.c_lo;
    o.tptr.assign(static_cast<size_t>(nc) + 1, 0);
    o.len.resize(static_cast<size_t>(o.n));
    uint64_t total = 0;
    for (int64_t i = 0; i < o.n; ++i) {
      const int32_t r = pl.rows[o.lo + i];
      const int64_t b = p.begin(r), e = p.end(r);
      int64_t lo = nc;
      for (int64_t j = b; j < e; ++j) {
        const int64_t c = static_cast<int64_t>(p.col[j]) - p.c_lo;
        if (c < 0 || c >= nc) return false;
        ++o.tptr[static_cast<size_t>(c) + 1];
        lo = std::min(lo, c);
      }
      key[o.lo + i] = static_cast<int32_t>(lo);
      o.len[static_cast<size_t>(i)] = static_cast<int32_t>(e - b);
      total += static_cast<uint64_t>(e - b);
    }
    if (total > 0xffffffffull) throw std::length_error("an owner's lists");
    for (size_t c = 0; c < static_cast<size_t>(nc); ++c) o.tptr[c + 1] += o.tptr[c];
    o.tl.resize(static_cast<size_t>(total));
    {
      std::vector<uint32_t> fill(o.tptr.begin(), o.tptr.end() - 1);
      for (int64_t i = 0; i < o.n; ++i) {
        const int32_t r = pl.rows[o.lo + i];
        for (int64_t j = p.begin(r), e = p.end(r); j < e; ++j)
          o.tl[fill[static_cast<size_t>(p.col[j] - p.c_lo)]++] = static_cast<int32_t>(i);
      }
    }
    o.cnt.assign(static_cast<size_t>(G) * static_cast<size_t>(o.n), 0);
    o.stack.assign(static_cast<size_t>(G) * static_cast<size_t>(pl.max_len + 1), {});
    o.top.assign(static_cast<size_t>(G), 0);
    o.mark.assign(static_cast<size_t>(o.n), 0);
    o.live = o.n;
    return true;
  }

  // Takes the placed rows out of the owner's transposed lists (they move no more, and by the middle
  // of the walk every other entry is one): whenever a quarter of the rows the lists hold are placed.
  template <class Cnt>
  void pack_lists(Owner<Cnt>& o) {
    const size_t nc = o.tptr.size() - 1;
    uint32_t w = 0, j = 0;
    for (size_t c = 0; c < nc; ++c) {
      const uint32_t e = o.tptr[c + 1];
      o.tptr[c] = w;
      for (; j < e; ++j)
        if (o.cnt[static_cast<size_t>(o.tl[j])] != Owner<Cnt>::kPlaced) o.tl[w++] = o.tl[j];
    }
    o.tptr[nc] = w;
    o.live -= o.gone;
    o.gone = 0;
  }

  // Adds the owner-local row t of length len to a proposal (shortest first, then lower row first)
  // unless it is there.
  inline void offer(Proposal& out, int32_t len32, int32_t row) {
    const uint16_t len = static_cast<uint16_t>(std::min<int32_t>(len32, 0xffff));
    for (int i = 0; i < out.n; ++i)
      if (out.row[i] == row) return;
    int at = out.n++;
    for (; at > 0 && (out.len[at - 1] > len || (out.len[at - 1] == len && out.row[at - 1] > row));
         --at) {
      out.len[at] = out.len[at - 1];
      out.row[at] = out.row[at - 1];
    }
    out.len[at] = len;
    out.row[at] = row;
  }

  // Keeps of stack b the good entries, each row's most recent one, in their order.
  template <class Cnt>
  void sweep(Owner<Cnt>& o, const Cnt* cn, std::vector<int32_t>& st, int32_t b) {
    size_t w = st.size();
    for (size_t i = st.size(); i-- > 0;) {
      const int32_t t = st[i];
      if (static_cast<int32_t>(cn[t]) != b || o.mark[static_cast<size_t>(t)]) continue;
      o.mark[static_cast<size_t>(t)] = 1;
      st[--w] = t;
    }
    for (size_t i = w; i < st.size(); ++i) o.mark[static_cast<size_t>(st[i])] = 0;
    st.erase(st.begin(), st.begin() + static_cast<std::ptrdiff_t>(w));
  }

  // The rows walker g's highest count offers at this owner: the kPickScan most recent of them.
  template <class Cnt>
  void propose(Owner<Cnt>& o, int g, int64_t max_len, const int32_t* recent, int64_t recent_n,
               Proposal& out) {
    const Cnt* const cn = o.cnt.data() + static_cast<size_t>(g) * static_cast<size_t>(o.n);
    std::vector<int32_t>* const stk =
        o.stack.data() + static_cast<size_t>(g) * static_cast<size_t>(max_len + 1);
    int32_t top = o.top[static_cast<size_t>(g)];
    for (; top >= 2; --top) {
      std::vector<int32_t>& st = stk[top];
      while (!st.empty() && static_cast<int32_t>(cn[st.back()]) != top) st.pop_back();
      if (!st.empty()) break;
    }
    o.top[static_cast<size_t>(g)] = top;
    out.n = 0;
    if (top >= 2) {
      out.cnt = top;
      const std::vector<int32_t>& st = stk[top];
      const size_t stop = st.size() > kStackLook ? st.size() - kStackLook : 0;
      for (size_t i = st.size(); i-- > stop && out.n < kPickScan;) {
        const int32_t t = st[i];
        if (static_cast<int32_t>(cn[t]) == top)
          offer(out, o.len[static_cast<size_t>(t)], static_cast<int32_t>(o.lo + t));
      }
      return;
    }
    // count 1: the unplaced rows of the columns that last came into the walker's window
    out.cnt = 1;
    const int64_t back = std::min<int64_t>(recent_n, kRecentCols);
    for (int64_t q = 1; q <= back && out.n < kPickScan; ++q) {
      const size_t c = static_cast<size_t>(recent[(recent_n - q) % kRecentCols]);
      for (uint32_t j = o.tptr[c], e = o.tptr[c + 1]; j < e && out.n < kPickScan; ++j) {
        const int32_t t = o.tl[j];
        if (cn[t] != Owner<Cnt>::kPlaced && cn[t] >= 1)
          offer(out, o.len[static_cast<size_t>(t)], static_cast<int32_t>(o.lo + t));
      }
    }
  }

  // Applies the round's column events, walker by walker, to the owner's rows. The lists and the
  // counts lie all over the owner's tables and a move waits for little else, so the events are
  // first unrolled into moves (walker, row, direction), every load asked for a fixed number of
  // steps ahead of its use.
  template <class Cnt>
  void apply_round(Owner<Cnt>& o, int G, int64_t max_len,
                   const std::vector<std::vector<uint32_t>>& events, std::vector<uint64_t>& evs,
                   std::vector<uint64_t>& moves) {
    constexpr size_t kAhead = 8, kMoveAhead = 16;
    evs.clear();
    moves.clear();
    for (int g = 0; g < G; ++g)
      for (const uint32_t ev : events[static_cast<size_t>(g)])
        evs.push_back(static_cast<uint64_t>(ev) << 16 | static_cast<uint64_t>(g));
    const uint32_t* const tptr = o.tptr.data();
    const int32_t* const tl = o.tl.data();
    const size_t ne = evs.size();
    for (size_t i = 0; i < std::min(ne, 2 * kAhead); ++i) __builtin_prefetch(tptr + (evs[i] >> 17));
    for (size_t i = 0; i < std::min(ne, kAhead); ++i) __builtin_prefetch(tl + tptr[evs[i] >> 17]);
    for (size_t i = 0; i < ne; ++i) {
      if (i + 2 * kAhead < ne) __builtin_prefetch(tptr + (evs[i + 2 * kAhead] >> 17));
      if (i + kAhead < ne) __builtin_prefetch(tl + tptr[evs[i + kAhead] >> 17]);
      const size_t c = static_cast<size_t>(evs[i] >> 17);
      const uint64_t low = (evs[i] & 0xffffu) << 1 | (evs[i] >> 16 & 1u);  // walker · 2 + direction
      for (uint32_t j = tptr[c], e = tptr[c + 1]; j < e; ++j)
        moves.push_back(static_cast<uint64_t>(static_cast<uint32_t>(tl[j])) << 32 | low);
    }
    Cnt* const cnt = o.cnt.data();
    const size_t n = static_cast<size_t>(o.n), nm = moves.size();
    const size_t sweep_at = 2 * n + 256;
    auto at = [&](uint64_t mv) { return cnt + (mv >> 1 & 0xffffu) * n + (mv >> 32); };
    for (size_t i = 0; i < std::min(nm, kMoveAhead); ++i) __builtin_prefetch(at(moves[i]), 1);
    for (size_t i = 0; i < nm; ++i) {
      if (i + kMoveAhead < nm) __builtin_prefetch(at(moves[i + kMoveAhead]), 1);
      const uint64_t mv = moves[i];
      Cnt* const cn = at(mv);
      const Cnt b = *cn;
      if (b == Owner<Cnt>::kPlaced) continue;
      int32_t to;  // the stack the row comes to, if it keeps one
      if (mv & 1u) {
        *cn = static_cast<Cnt>(b + 1);
        if (b < 1) continue;
        to = static_cast<int32_t>(b) + 1;
      } else {
        // (an unplaced row that holds a counted column of the window has b >= 1)
        if (b < 1) continue;
        *cn = static_cast<Cnt>(b - 1);
        if (b < 3) continue;
        to = static_cast<int32_t>(b) - 1;
      }
      const size_t g = mv >> 1 & 0xffffu;
      std::vector<int32_t>& st =
          o.stack[g * static_cast<size_t>(max_len + 1) + static_cast<size_t>(to)];
      if (st.size() >= sweep_at) sweep(o, cnt + g * n, st, to);
      st.push_back(static_cast<int32_t>(mv >> 32));
      if ((mv & 1u) && to > o.top[g]) o.top[g] = to;
    }
  }

  // Member `me` of `team` walks the pool with its peers. Returns what went wrong: 0 nothing, 1 a
  // column out of range, 2 no memory (the same answer at every member).
  template <class Cnt>
  int walk_pool(Team& team, int me, const Pool& pl, int64_t window, int64_t col_cap) {
    const int G = static_cast<int>(pl.size.size());
    const int K = pl.K, T = team.size;
    const Pieces& p = pl.p;
    const int64_t nc = p.c_hi - p.c_lo, m = pl.m;
    const int k_lo = K * me / T, k_hi = K * (me + 1) / T;  // this member's owners
    window = std::min<int64_t>(window, std::max<int64_t>(1, pl.nnz));

    if (me == 0) {
      PoolState<Cnt>* made = nullptr;
      try {
        made = new PoolState<Cnt>();
        made->owners.resize(static_cast<size_t>(K));
        for (int k = 0; k < K; ++k) {
          made->owners[static_cast<size_t>(k)].lo = m * k / K;
          made->owners[static_cast<size_t>(k)].n = m * (k + 1) / K - m * k / K;
        }
        made->key.resize(static_cast<size_t>(m));
        made->by_min.resize(static_cast<size_t>(m));
        made->coldeg.assign(static_cast<size_t>(nc), 0);
        made->placed.assign(static_cast<size_t>(m), 0);
        made->in_fifo.assign(static_cast<size_t>(G) * static_cast<size_t>(nc), 0);
        made->fifo.resize(static_cast<size_t>(G));
        for (int g = 0; g < G; ++g)
          made->fifo[static_cast<size_t>(g)].resize(
              static_cast<size_t>(std::min(window, pl.size[static_cast<size_t>(g)] * pl.max_len)));
        made->fifo_at.assign(static_cast<size_t>(G), 0);
        made->fifo_n.assign(static_cast<size_t>(G), 0);
        made->events.resize(static_cast<size_t>(G));
        made->recent.assign(static_cast<size_t>(G) * kRecentCols, 0);
        made->recent_n.assign(static_cast<size_t>(G), 0);
        made->prop.resize(static_cast<size_t>(K) * static_cast<size_t>(G));
      } catch (const std::exception&) {
        delete made;
        made = nullptr;
      }
      team.state = made;
    }
    team.barrier.wait();
    PoolState<Cnt>* const st = static_cast<PoolState<Cnt>*>(team.state);
    if (!st) {
      team.barrier.wait();  // (member 0 writes team.state again at the next pool)
      return 2;
    }

    // the owners' tables
    for (int k = k_lo; k < k_hi; ++k) {
      try {
        if (!build_owner(pl, G, st->owners[static_cast<size_t>(k)], st->key.data()))
          st->bad_column.store(1);
      } catch (const std::exception&) {
        st->no_memory.store(1);
      }
    }
    team.barrier.wait();
    int bad = st->bad_column.load() ? 1 : st->no_memory.load() ? 2 : 0;
    if (!bad) {
      // a column's entries in the pool, and the fall-back order (ascending smallest column, ties in
      // natural order: a counting sort over the keys)
      for (int64_t c = nc * me / T, e = nc * (me + 1) / T; c < e; ++c) {
        int64_t deg = 0;
        for (int k = 0; k < K; ++k) {
          const Owner<Cnt>& o = st->owners[static_cast<size_t>(k)];
          deg += o.tptr[static_cast<size_t>(c) + 1] - o.tptr[static_cast<size_t>(c)];
        }
        st->coldeg[static_cast<size_t>(c)] =
            static_cast<int32_t>(std::min<int64_t>(deg, 0x7fffffff));
      }
      if (me == T - 1) {
      try {
          std::vector<int64_t> at(static_cast<size_t>(nc) + 2, 0);
          const int32_t* const key = st->key.data();
          for (int64_t i = 0; i < m; ++i) ++at[static_cast<size_t>(key[i]) + 1];
          for (size_t c = 0; c <= static_cast<size_t>(nc); ++c) at[c + 1] += at[c];
          for (int64_t i = 0; i < m; ++i)
            st->by_min[static_cast<size_t>(at[static_cast<size_t>(key[i])]++)] =
                static_cast<int32_t>(i);
      } catch (const std::exception&) {
        st->no_memory.store(1);
      }
    }
    team.barrier.wait();
    bad = st->no_memory.load() ? 2 : 0;
  }

  if (!bad) {
    // (window / kRoundShare gathers, in rows of the pool's mean length)
    const int64_t B = std::clamp<int64_t>(window * m / (kRoundShare * pl.nnz), 1, kMaxRowsPerRound);
    int64_t longest = 0;
    for (int g = 0; g < G; ++g) longest = std::max(longest, pl.size[static_cast<size_t>(g)]);
    int64_t fall = 0;  // every member keeps its own, and they agree
    std::vector<int32_t> pick;         // [B][G]
    std::vector<uint64_t> evs, moves;  // apply_round's scratch
    try {
      pick.resize(static_cast<size_t>(G) * static_cast<size_t>(B));
    } catch (const std::exception&) {
      st->fail_apply.store(1);
    }
    const uint8_t* const placed = st->placed.data();
    const int32_t* const by_min = st->by_min.data();
    for (int64_t s0 = 0; s0 < longest; s0 += B) {
      // 1. what this member's owners offer every walker
      for (int k = k_lo; k < k_hi; ++k)
        for (int g = 0; g < G; ++g)
          if (s0 < pl.size[static_cast<size_t>(g)])
            propose(st->owners[static_cast<size_t>(k)], g, pl.max_len,
                    st->recent.data() + static_cast<size_t>(g) * kRecentCols,
                    st->recent_n[static_cast<size_t>(g)],
                    st->prop[static_cast<size_t>(g) * static_cast<size_t>(K) +
                             static_cast<size_t>(k)]);
      team.barrier.wait();
      if (st->fail_apply.load()) break;
      // 2. the picks, row by row and walker by walker (the same at every member)
      for (size_t i = 0; i < st->prop.size(); ++i) __builtin_prefetch(&st->prop[i]);
      size_t n_pick = 0;
      auto taken = [&](int32_t row) {
        for (size_t h = 0; h < n_pick; ++h)
          if (pick[h] == row) return true;
        return false;
      };
      for (int64_t s = s0; s < s0 + B; ++s)
        for (int g = 0; g < G; ++g, ++n_pick) {
          pick[n_pick] = -1;
          if (s >= pl.size[static_cast<size_t>(g)]) continue;
          int32_t best = -1, best_cnt = 0, best_len = 0;
          for (int k = 0; k < K; ++k) {
            const Proposal& pr = st->prop[static_cast<size_t>(g) * static_cast<size_t>(K) +
                                          static_cast<size_t>(k)];
            if (pr.n == 0 || (best >= 0 && pr.cnt < best_cnt)) continue;
            for (int i = 0; i < pr.n; ++i) {
              if (taken(pr.row[i])) continue;
              // (owners ascend with their rows: of equals the first one met is the lower row)
              if (best < 0 || pr.cnt > best_cnt || pr.len[i] < best_len) {
                best = pr.row[i];
                best_cnt = pr.cnt;
                best_len = pr.len[i];
              }
              break;
            }
          }
          if (best < 0) {
            while (placed[by_min[fall]] || taken(by_min[fall])) ++fall;
            best = by_min[fall];
          }
          pick[n_pick] = best;
        }
      // ... and the FIFOs of the walkers this member keeps
      try {
        for (int g = me; g < G; g += T) {
          std::vector<uint32_t>& ev = st->events[static_cast<size_t>(g)];
          ev.clear();
          int32_t* const fifo = st->fifo[static_cast<size_t>(g)].data();
          const int64_t cap = static_cast<int64_t>(st->fifo[static_cast<size_t>(g)].size());
          int32_t* const in_fifo =
              st->in_fifo.data() + static_cast<size_t>(g) * static_cast<size_t>(nc);
          int64_t& fifo_at = st->fifo_at[static_cast<size_t>(g)];
          int64_t& fifo_n = st->fifo_n[static_cast<size_t>(g)];
          int32_t* const recent = st->recent.data() + static_cast<size_t>(g) * kRecentCols;
          int64_t& recent_n = st->recent_n[static_cast<size_t>(g)];
          for (int64_t i = 0; i < B; ++i) {
            const int32_t at = pick[static_cast<size_t>(i) * static_cast<size_t>(G) +
                                    static_cast<size_t>(g)];
            if (at < 0) continue;
            const int32_t r = pl.rows[at];
            pl.seq[pl.off[static_cast<size_t>(g)] + s0 + i] = r;
            for (int64_t j = p.begin(r), e = p.end(r); j < e; ++j) {
              const int64_t c = static_cast<int64_t>(p.col[j]) - p.c_lo;
              int64_t slot;
              if (fifo_n == cap) {  // the oldest gather leaves
                const int64_t o = fifo[fifo_at];
                if (--in_fifo[o] == 0 && st->coldeg[static_cast<size_t>(o)] <= col_cap)
                  ev.push_back(static_cast<uint32_t>(o) << 1);
                slot = fifo_at;
                fifo_at = fifo_at + 1 == cap ? 0 : fifo_at + 1;
              } else {
                slot = fifo_at + fifo_n;
                if (slot >= cap) slot -= cap;
                ++fifo_n;
              }
              fifo[slot] = static_cast<int32_t>(c);
              if (in_fifo[c]++ == 0 && st->coldeg[static_cast<size_t>(c)] <= col_cap) {
                ev.push_back((static_cast<uint32_t>(c) << 1) | 1u);
                recent[recent_n++ % kRecentCols] = static_cast<int32_t>(c);
              }
            }
          }
        }
      } catch (const std::exception&) {
        st->fail_fifo.store(1);
      }
      team.barrier.wait();
      if (st->fail_fifo.load()) break;
      // 3. the owners take the picked rows out and move their rows by the columns' events
      try {
        for (int k = k_lo; k < k_hi; ++k) {
          Owner<Cnt>& o = st->owners[static_cast<size_t>(k)];
          for (size_t h = 0; h < n_pick; ++h) {
            const int64_t t = static_cast<int64_t>(pick[h]) - o.lo;
            if (pick[h] < 0 || t < 0 || t >= o.n) continue;
            for (int g = 0; g < G; ++g)
              o.cnt[static_cast<size_t>(g) * static_cast<size_t>(o.n) + static_cast<size_t>(t)] =
                  Owner<Cnt>::kPlaced;
            st->placed[static_cast<size_t>(o.lo + t)] = 1;
            ++o.gone;
          }
          if (o.gone >= 64 && o.gone * 4 >= o.live) pack_lists(o);
          apply_round(o, G, pl.max_len, st->events, evs, moves);
        }
      } catch (const std::exception&) {
        st->fail_apply.store(1);
      }
    }
  }
  team.barrier.wait();
  if (st->fail_apply.load() || st->fail_fifo.load()) bad = 2;
  team.barrier.wait();
  if (me == 0) {
    delete st;
    team.state = nullptr;
  }
  return bad;
}

int walk_pool_any(Team& team, int me, const Pool& pl, int64_t window, int64_t col_cap) {
  if (pl.max_len < 0xff) return walk_pool<uint8_t>(team, me, pl, window, col_cap);
  if (pl.max_len < 0xffff) return walk_pool<uint16_t>(team, me, pl, window, col_cap);
  return walk_pool<int32_t>(team, me, pl, window, col_cap);
}

// The pools of one walk over the non-empty rows ne[0, m): the parts of add_tasks, G XCDs to a
// pool (G divides X), every part's walker writing its part of seq[0, m).
void add_pools(const Pieces& p, const int32_t* ne, int64_t m, int64_t R, int64_t X, int64_t G,
               int32_t* seq, std::vector<Pool>& pools, std::vector<int64_t>& part_off) {
  std::vector<Task> unused;
  add_tasks(p, ne, m, R, X, 1, seq, unused, part_off);
  for (int64_t q = 0; q < X / G; ++q) {
    const int64_t b = part_off[static_cast<size_t>(q * G)];
    const int64_t e = part_off[static_cast<size_t>((q + 1) * G)];
    if (e == b) continue;
    Pool pl{p, ne + b, e - b, seq + b, {}, {}, 0, 0, 1};
    for (int64_t g = 0; g < G; ++g) {
      pl.off.push_back(part_off[static_cast<size_t>(q * G + g)] - b);
      pl.size.push_back(part_off[static_cast<size_t>(q * G + g) + 1] -
                        part_off[static_cast<size_t>(q * G + g)]);
    }
    for (int64_t i = b; i < e; ++i) {
      const int64_t len = p.end(ne[i]) - p.begin(ne[i]);
      pl.nnz += len;
      pl.max_len = std::max(pl.max_len, len);
    }
    // at least two entries of a column to an owner (more owners would find most lists empty)
    const int64_t deg = pl.nnz / std::max<int64_t>(1, p.c_hi - p.c_lo);
    while (pl.K * 2 <= kMaxOwners && pl.K * 4 <= deg) pl.K *= 2;
    pools.push_back(std::move(pl));
  }
}

// Walks the pools on up to `threads` threads: as many teams as there are pools (at most one to a
// thread), team i taking pools i, i + teams, ...; a team's members run the pool's owners between
// them. As run_tasks: no exception leaves it, and a thread that cannot be started is done without.
hgd_status run_pools(const char* fn, const std::vector<Pool>& pools, int64_t window,
                     int64_t col_cap, int32_t threads) {
  if (pools.empty()) return HGD_OK;
  int64_t owners = 0;
  for (const Pool& pl : pools) owners += pl.K;
  std::atomic<int> bad_column{0}, no_memory{0};
  std::atomic<int> go{0};  // how many threads there are, once that is known (-1: none is to run)
  std::vector<std::unique_ptr<Team>> teams;
  auto work = [&](int id) noexcept {
    int n;
    for (int spin = 0; (n = go.load(std::memory_order_acquire)) == 0; ++spin)
      if (spin >= 512) std::this_thread::yield();
    if (n < 0) return;
    // thread id is member id / teams of team id % teams
    const int n_teams = static_cast<int>(teams.size());
    Team& team = *teams[static_cast<size_t>(id % n_teams)];
    for (size_t i = static_cast<size_t>(id % n_teams); i < pools.size();
         i += static_cast<size_t>(n_teams)) {
      const int bad = walk_pool_any(team, id / n_teams, pools[i], window, col_cap);
      if (bad == 1) bad_column.store(1);
      if (bad == 2) no_memory.store(1);
    }
  };
  int n = 1;
  std::vector<std::thread> th;
  try {
    const int want = pick_threads(threads, owners);
    th.reserve(static_cast<size_t>(want));
    for (int i = 1; i < want; ++i) {
      th.emplace_back(work, i);
      ++n;
    }
  } catch (const std::exception&) {  // (system_error: no more threads to be had)
  }
  try {
    const int n_teams = static_cast<int>(std::min<size_t>(pools.size(), static_cast<size_t>(n)));
    for (int i = 0; i < n_teams; ++i)
      teams.emplace_back(new Team(n / n_teams + (i < n % n_teams ? 1 : 0)));
  } catch (const std::exception&) {
    go.store(-1, std::memory_order_release);
    for (auto& t : th) t.join();
    return greedy_fail(HGD_ERR_WORKSPACE, "%s: out of host memory", fn);
  }
  go.store(n, std::memory_order_release);
  work(0);
  for (auto& t : th) t.join();
  if (bad_column.load())
    return greedy_fail(HGD_ERR_INVALID_ARG, "%s: a column outside [0, n_cols)", fn);
  if (no_memory.load()) return greedy_fail(HGD_ERR_WORKSPACE, "%s: out of host memory", fn);
  return HGD_OK;
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

// The row form of both walks: xcds_per_pool = 0 is the walk of every part's chunks on their own,
// otherwise chunks_per_xcd is 1 and the parts' walkers share pools.
hgd_status row_order(const char* fn, const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                     int64_t n_cols, int64_t window, int32_t col_cap, int32_t rows_per_wg,
                     int32_t n_xcd, int32_t chunks_per_xcd, int32_t xcds_per_pool, int32_t threads,
                     int32_t* order_out) {
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
    if (xcds_per_pool > 1) {
      std::vector<Pool> pools;
      add_pools(p, ne.data(), m, rows_per_wg, n_xcd, xcds_per_pool, seq.data(), pools, part_off);
      s = run_pools(fn, pools, window, col_cap, threads);
    } else {
      add_tasks(p, ne.data(), m, rows_per_wg, n_xcd, chunks_per_xcd, seq.data(), tasks, part_off);
      s = run_tasks(fn, tasks, window, col_cap, threads);
    }
    if (s != HGD_OK) return s;
    place_parts(seq.data(), part_off, rows_per_wg, n_xcd, order_out);
  } catch (const std::exception&) {
    return greedy_fail(HGD_ERR_WORKSPACE, "%s: out of host memory", fn);
  }
  return HGD_OK;
}

hgd_status block_order(const char* fn, const int64_t* rowptr, const int32_t* col, int64_t n_rows,
                       int64_t n_cols, int32_t n_blocks, int64_t window, int32_t col_cap,
                       int32_t rows_per_wg, int32_t n_xcd, int32_t chunks_per_xcd,
                       int32_t xcds_per_pool, int32_t threads, int32_t* blk_order_out) {
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
    std::vector<Pool> pools;
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
      if (xcds_per_pool > 1)
        add_pools(p, nek, mk, rows_per_wg, n_xcd, xcds_per_pool, seq.data() + k * n_rows, pools,
                  part_off[static_cast<size_t>(k)]);
      else
        add_tasks(p, nek, mk, rows_per_wg, n_xcd, chunks_per_xcd, seq.data() + k * n_rows, tasks,
                  part_off[static_cast<size_t>(k)]);
    }
    s = xcds_per_pool > 1 ? run_pools(fn, pools, window, col_cap, threads)
                          : run_tasks(fn, tasks, window, col_cap, threads);
    if (s != HGD_OK) return s;
    for (int64_t k = 0; k < P; ++k)
      place_parts(seq.data() + k * n_rows, part_off[static_cast<size_t>(k)], rows_per_wg, n_xcd,
                  blk_order_out + k * n_rows);
  } catch (const std::exception&) {
    return greedy_fail(HGD_ERR_WORKSPACE, "%s: out of host memory", fn);
  }
  return HGD_OK;
}

// A pool width must divide n_xcd (checked after the arguments both forms share).
hgd_status check_pool(const char* fn, int32_t n_xcd, int32_t xcds_per_pool) {
  if (xcds_per_pool < 1 || n_xcd < 1 || n_xcd % xcds_per_pool != 0)
    return greedy_fail(HGD_ERR_INVALID_ARG,
                       "%s: n_xcd and xcds_per_pool must be >= 1, and the second divide the first",
                       fn);
  if (xcds_per_pool > 64)
    return greedy_fail(HGD_ERR_INVALID_ARG, "%s: xcds_per_pool must be <= 64", fn);
  return HGD_OK;
}

}  // namespace
}  // namespace hgd

extern "C" hgd_status hgd_row_order_greedy(const int64_t* rowptr, const int32_t* col,
                                           int64_t n_rows, int64_t n_cols, int64_t window,
                                           int32_t col_cap, int32_t rows_per_wg, int32_t n_xcd,
                                           int32_t chunks_per_xcd, int32_t threads,
                                           int32_t* order_out) {
  return hgd::row_order("hgd_row_order_greedy", rowptr, col, n_rows, n_cols, window, col_cap,
                        rows_per_wg, n_xcd, chunks_per_xcd, 0, threads, order_out);
}

extern "C" hgd_status hgd_col_block_order_greedy(const int64_t* rowptr, const int32_t* col,
                                                 int64_t n_rows, int64_t n_cols, int32_t n_blocks,
                                                 int64_t window, int32_t col_cap,
                                                 int32_t rows_per_wg, int32_t n_xcd,
                                                 int32_t chunks_per_xcd, int32_t threads,
                                                 int32_t* blk_order_out) {
  return hgd::block_order("hgd_col_block_order_greedy", rowptr, col, n_rows, n_cols, n_blocks,
                          window, col_cap, rows_per_wg, n_xcd, chunks_per_xcd, 0, threads,
                          blk_order_out);
}

extern "C" hgd_status hgd_row_order_greedy_pooled(const int64_t* rowptr, const int32_t* col,
                                                  int64_t n_rows, int64_t n_cols, int64_t window,
                                                  int32_t col_cap, int32_t rows_per_wg,
                                                  int32_t n_xcd, int32_t xcds_per_pool,
                                                  int32_t threads, int32_t* order_out) {
  constexpr const char* fn = "hgd_row_order_greedy_pooled";
  hgd::g_last_error[0] = '\0';
  if (hgd::check_pool(fn, n_xcd, xcds_per_pool) != HGD_OK) return HGD_ERR_INVALID_ARG;
  return hgd::row_order(fn, rowptr, col, n_rows, n_cols, window, col_cap, rows_per_wg, n_xcd, 1,
                        xcds_per_pool, threads, order_out);
}

extern "C" hgd_status hgd_col_block_order_greedy_pooled(
    const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_cols, int32_t n_blocks,
    int64_t window, int32_t col_cap, int32_t rows_per_wg, int32_t n_xcd, int32_t xcds_per_pool,
    int32_t threads, int32_t* blk_order_out) {
  constexpr const char* fn = "hgd_col_block_order_greedy_pooled";
  hgd::g_last_error[0] = '\0';
  if (hgd::check_pool(fn, n_xcd, xcds_per_pool) != HGD_OK) return HGD_ERR_INVALID_ARG;
  return hgd::block_order(fn, rowptr, col, n_rows, n_cols, n_blocks, window, col_cap, rows_per_wg,
                          n_xcd, 1, xcds_per_pool, threads, blk_order_out);
}
