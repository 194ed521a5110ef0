// Stand-alone driver of the pooled walk of csrc/row_order_greedy.cpp for sanitizer builds (address
// + undefined, thread): compiled together with that file, no HIP, no Python. Runs
// hgd_row_order_greedy_pooled and hgd_col_block_order_greedy_pooled over small graphs — empty
// rows, a column over the cap, a short last workgroup — at every pool width and with 1 to 16
// threads (the round barriers are what the thread build is for), and checks that every order is a
// permutation, does not depend on the thread count, and at a pool width of 1 is
// hgd_row_order_greedy's. Exit status 0 when all is well.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/hgd.h"

namespace hgd {
thread_local char g_last_error[512] = {0};  // (the library's is structure.hip's)
}

namespace {

struct Graph {
  std::vector<int64_t> rowptr;
  std::vector<int32_t> col;
  int64_t n_rows, n_cols;
};

uint64_t next(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

// Rows of 0..12 ascending columns (every 7th row empty), and column 0 in every third row: more
// entries than the cap the runs below use.
Graph make_graph(int64_t n_rows, int64_t n_cols, uint64_t seed) {
  Graph g{{0}, {}, n_rows, n_cols};
  uint64_t s = seed * 2654435761ull + 1;
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t len = r % 7 == 3 ? 0 : static_cast<int64_t>(next(s) % 13);
    std::vector<char> has(static_cast<size_t>(n_cols), 0);
    if (len > 0 && r % 3 == 0) has[0] = 1;
    for (int64_t k = 0; k < len; ++k) has[static_cast<size_t>(next(s) % n_cols)] = 1;
    for (int64_t c = 0; c < n_cols; ++c)
      if (has[static_cast<size_t>(c)]) g.col.push_back(static_cast<int32_t>(c));
    g.rowptr.push_back(static_cast<int64_t>(g.col.size()));
  }
  return g;
}

bool is_permutation(const int32_t* p, int64_t n) {
  std::vector<char> seen(static_cast<size_t>(n), 0);
  for (int64_t i = 0; i < n; ++i) {
    if (p[i] < 0 || p[i] >= n || seen[static_cast<size_t>(p[i])]) return false;
    seen[static_cast<size_t>(p[i])] = 1;
  }
  return true;
}

int fails = 0;

void expect(bool ok, const char* what, int64_t n, int r, int pool, int threads) {
  if (ok) return;
  ++fails;
  std::fprintf(stderr, "FAILED %s: n_rows %lld, rows_per_wg %d, pool %d, threads %d (%s)\n", what,
               static_cast<long long>(n), r, pool, threads, hgd::g_last_error);
}

}  // namespace

int main() {
  const int64_t sizes[] = {0, 1, 17, 129, 8 * 16 * 3 + 5};
  const int rs[] = {8, 16};
  const int pools[] = {1, 2, 4, 8};
  const int blocks[] = {2, 3};
  for (int64_t n : sizes) {
    const Graph g = make_graph(n, 61, static_cast<uint64_t>(n) + 1);
    for (int r : rs)
      for (int pool : pools) {
        std::vector<int32_t> first;
        // (every count from 1 to 16 at the two larger graphs, the ends below)
        for (int threads = 1; threads <= 16; threads += (n < 129 && threads > 1 ? 7 : 1)) {
          std::vector<int32_t> order(static_cast<size_t>(n) + 1, -1);
          const hgd_status s =
              hgd_row_order_greedy_pooled(g.rowptr.data(), g.col.data(), n, g.n_cols, 64, 4, r, 8,
                                          pool, threads, order.data());
          expect(s == HGD_OK, "hgd_row_order_greedy_pooled", n, r, pool, threads);
          expect(order[static_cast<size_t>(n)] == -1 && is_permutation(order.data(), n),
                 "row order is a permutation", n, r, pool, threads);
          if (first.empty()) first = order;
          expect(order == first, "row order by thread count", n, r, pool, threads);
        }
        if (pool == 1) {
          std::vector<int32_t> order(static_cast<size_t>(n) + 1, -1);
          expect(hgd_row_order_greedy(g.rowptr.data(), g.col.data(), n, g.n_cols, 64, 4, r, 8, 1, 1,
                                      order.data()) == HGD_OK && order == first,
                 "a pool of one XCD is the part walked alone", n, r, pool, 1);
        }
        for (int P : blocks) {
          std::vector<int32_t> first_blk;
          for (int threads : {1, 2, 3, 5, 8, 16}) {
            std::vector<int32_t> order(static_cast<size_t>(n) * P + 1, -1);
            const hgd_status s = hgd_col_block_order_greedy_pooled(
                g.rowptr.data(), g.col.data(), n, g.n_cols, P, 64, 4, r, 8, pool, threads,
                order.data());
            expect(s == HGD_OK, "hgd_col_block_order_greedy_pooled", n, r, pool, threads);
            bool perm = order[static_cast<size_t>(n) * P] == -1;
            for (int k = 0; k < P; ++k) perm = perm && is_permutation(order.data() + k * n, n);
            expect(perm, "block orders are permutations", n, r, pool, threads);
            if (first_blk.empty()) first_blk = order;
            expect(order == first_blk, "block orders by thread count", n, r, pool, threads);
          }
        }
      }
  }
  // a window that never fills: the walkers take several rows a round
  {
    const int64_t n = 2005;
    const Graph g = make_graph(n, 61, 77);
    for (int pool : pools) {
      std::vector<int32_t> first;
      for (int threads : {1, 2, 5, 16}) {
        std::vector<int32_t> order(static_cast<size_t>(n) + 1, -1);
        const hgd_status s = hgd_row_order_greedy_pooled(g.rowptr.data(), g.col.data(), n,
                                                         g.n_cols, 1 << 20, 4, 16, 8, pool,
                                                         threads, order.data());
        expect(s == HGD_OK && order[static_cast<size_t>(n)] == -1 &&
                   is_permutation(order.data(), n),
               "long window: row order is a permutation", n, 16, pool, threads);
        if (first.empty()) first = order;
        expect(order == first, "long window: row order by thread count", n, 16, pool, threads);
      }
    }
  }
  // a column outside the structure and a pool that does not divide the XCDs are refused
  {
    const int64_t rowptr[] = {0, 2};
    const int32_t col[] = {1, 99};
    int32_t order[2] = {-1, -1};
    for (int pool : pools) {
      expect(hgd_row_order_greedy_pooled(rowptr, col, 1, 10, 64, 16, 16, 8, pool, 2, order) ==
                 HGD_ERR_INVALID_ARG, "column out of range", 1, 16, pool, 2);
      expect(hgd_col_block_order_greedy_pooled(rowptr, col, 1, 10, 2, 64, 16, 16, 8, pool, 2,
                                               order) == HGD_ERR_INVALID_ARG,
             "column out of range (blocks)", 1, 16, pool, 2);
    }
    expect(hgd_row_order_greedy_pooled(rowptr, col, 1, 100, 64, 16, 16, 8, 3, 1, order) ==
               HGD_ERR_INVALID_ARG, "pool of 3 of 8 XCDs", 1, 16, 3, 1);
  }
  if (fails) return 1;
  std::puts("row_order_pooled: all orders are permutations, whatever the thread count");
  return 0;
}
