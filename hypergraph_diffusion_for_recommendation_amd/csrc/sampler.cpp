// Host-side pairwise sampler, bit-identical to the reference's Python one.
//
// Reference (paths relative to /root/reference/HD_SELFRec): next_batch_pairwise
// (util/sampler.py:237-264) shuffles data.training_data IN PLACE with random.shuffle, then for
// every record of a batch draws n_negs negatives with random.choice(item_list), redrawing while
// the item is in the user's training items. Every training epoch of every plugin runs this
// Python loop (≈ 3 µs per record: seconds per epoch at Yelp2018 size, more than the device
// step it feeds).
//
// This file restates CPython's generator exactly — MT19937 (Modules/_randommodule.c
// genrand_uint32), getrandbits(k) = genrand_uint32() >> (32 - k) for k <= 32, and
// Random._randbelow_with_getrandbits(n) (k = n.bit_length(), redraw while r >= n), which both
// shuffle (j = randbelow(i + 1), i = n-1 .. 1) and choice (seq[randbelow(len(seq))]) use — on the
// state random.getstate() exposes (624 words + position), so the caller can hand the state in
// and back (random.setstate) and the Python random stream continues exactly as if the reference
// loop had run. item_list = list(data.item.keys()) is the dense item order, so the choice index
// IS the dense id; membership is a binary search in the user's sorted training items.
//
// next_batch_unified (util/sampler.py:7-90), the KG carriers' generator, adds three things on
// top of that loop, restated here as well:
//  * its two epoch shuffles run random.shuffle on 2-D NumPy arrays, whose rows are views: the
//    swap degenerates to x[i] = x[j] (hgd_py_shuffle_rows);
//  * np.random.randint(n, size=k) on NumPy's global legacy RandomState: the same MT19937
//    (np.random.get_state() exposes key and position), 32-bit outputs masked to the bit length of
//    n - 1 and redrawn while above it, nothing drawn for n == 1;
//  * random.choice(all_tails) redrawn while in the head's tail set: a binary search in the head's
//    sorted distinct tails (hgd_sample_unified).
#include <cstdint>
#include <cstring>

#include "../../include/hgd.h"
#include "hgd_internal.h"

namespace hgd {
namespace {

constexpr int kMtN = 624;
constexpr int kMtM = 397;

struct Mt {
  uint32_t* mt;  // 624 words
  uint32_t index;

  uint32_t next() {
    static const uint32_t mag01[2] = {0x0u, 0x9908b0dfu};
    if (index >= static_cast<uint32_t>(kMtN)) {
      int kk;
      uint32_t y;
      for (kk = 0; kk < kMtN - kMtM; ++kk) {
        y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
        mt[kk] = mt[kk + kMtM] ^ (y >> 1) ^ mag01[y & 1u];
      }
      for (; kk < kMtN - 1; ++kk) {
        y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
        mt[kk] = mt[kk + (kMtM - kMtN)] ^ (y >> 1) ^ mag01[y & 1u];
      }
      y = (mt[kMtN - 1] & 0x80000000u) | (mt[0] & 0x7fffffffu);
      mt[kMtN - 1] = mt[kMtM - 1] ^ (y >> 1) ^ mag01[y & 1u];
      index = 0;
    }
    uint32_t y = mt[index++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }

  // Random._randbelow_with_getrandbits(n), 1 <= n < 2^32
  uint32_t below(uint64_t n) {
    int k = 0;
    while ((n >> k) != 0) ++k;  // n.bit_length()
    uint64_t r = k >= 32 ? next() : (next() >> (32 - k));
    while (r >= n) r = k >= 32 ? next() : (next() >> (32 - k));
    return static_cast<uint32_t>(r);
  }
};

bool sorted_contains(const int32_t* a, int64_t lo, int64_t hi, int32_t v) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] == v) return true;
    if (a[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return false;
}

hgd_status check_state(const uint32_t* state) {
  if (!state) return fail(HGD_ERR_INVALID_ARG, "null MT19937 state");
  if (state[kMtN] > static_cast<uint32_t>(kMtN))
    return fail(HGD_ERR_INVALID_ARG, "MT19937 position %u > 624", state[kMtN]);
  return HGD_OK;
}

// The CF part of a batch (sampler.py:47-54): shared by the pairwise and the unified sampler.
template <typename Out>
hgd_status sample_cf(const char* who, Mt& g, uint32_t* mt_state, const int64_t* order,
                     int64_t begin, int64_t end, const int32_t* rec_user, const int32_t* rec_item,
                     const int64_t* user_rowptr, const int32_t* user_items, int64_t n_users,
                     int64_t n_items, int32_t n_negs, Out* out_u, Out* out_i, Out* out_j) {
  for (int64_t k = begin; k < end; ++k) {
    const int64_t rec = order[k];
    const int32_t u = rec_user[rec];
    if (u < 0 || u >= n_users) {
      mt_state[kMtN] = g.index;
      return fail(HGD_ERR_INVALID_ARG, "%s: user id %d out of range", who, u);
    }
    out_u[k - begin] = u;
    out_i[k - begin] = rec_item[rec];
    const int64_t lo = user_rowptr[u], hi = user_rowptr[u + 1];
    if (hi - lo >= n_items && n_negs > 0) {  // the reference would loop forever
      mt_state[kMtN] = g.index;
      return fail(HGD_ERR_INVALID_ARG, "%s: user %d has interacted with every item", who, u);
    }
    for (int32_t m = 0; m < n_negs; ++m) {
      int32_t neg = static_cast<int32_t>(g.below(static_cast<uint64_t>(n_items)));
      while (sorted_contains(user_items, lo, hi, neg))
        neg = static_cast<int32_t>(g.below(static_cast<uint64_t>(n_items)));
      out_j[(k - begin) * n_negs + m] = neg;
    }
  }
  return HGD_OK;
}

bool sorted_contains64(const int64_t* a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] == v) return true;
    if (a[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return false;
}

}  // namespace
}  // namespace hgd

extern "C" hgd_status hgd_py_shuffle(uint32_t* mt_state, int64_t* order, int64_t n) {
  using namespace hgd;
  clear_error();
  hgd_status s = check_state(mt_state);
  if (s != HGD_OK) return s;
  HGD_REQUIRE(n >= 0 && n < (int64_t{1} << 32), "hgd_py_shuffle: n out of range");
  HGD_REQUIRE(order || n == 0, "hgd_py_shuffle: null order");
  Mt g{mt_state, mt_state[kMtN]};
  for (int64_t i = n - 1; i >= 1; --i) {  // random.shuffle: reversed(range(1, len(x)))
    const int64_t j = g.below(static_cast<uint64_t>(i) + 1);
    const int64_t t = order[i];
    order[i] = order[j];
    order[j] = t;
  }
  mt_state[kMtN] = g.index;
  return HGD_OK;
}

extern "C" hgd_status hgd_py_shuffle_rows(uint32_t* mt_state, int64_t* order, int64_t n) {
  using namespace hgd;
  clear_error();
  hgd_status s = check_state(mt_state);
  if (s != HGD_OK) return s;
  HGD_REQUIRE(n >= 0 && n < (int64_t{1} << 32), "hgd_py_shuffle_rows: n out of range");
  Mt g{mt_state, mt_state[kMtN]};
  // x[i], x[j] = x[j], x[i] on rows that are views: x[i] = x[j] copies row j over row i, then
  // x[j] = (the view of row i, which now holds row j) changes nothing
  for (int64_t i = n - 1; i >= 1; --i) {
    const int64_t j = g.below(static_cast<uint64_t>(i) + 1);
    if (order) order[i] = order[j];
  }
  mt_state[kMtN] = g.index;
  return HGD_OK;
}

extern "C" hgd_status hgd_sample_pairwise(uint32_t* mt_state, const int64_t* order, int64_t begin,
                                          int64_t end, const int32_t* rec_user,
                                          const int32_t* rec_item, const int64_t* user_rowptr,
                                          const int32_t* user_items, int64_t n_users,
                                          int64_t n_items, int32_t n_negs, int32_t* out_u,
                                          int32_t* out_i, int32_t* out_j) {
  using namespace hgd;
  clear_error();
  hgd_status s = check_state(mt_state);
  if (s != HGD_OK) return s;
  HGD_REQUIRE(begin >= 0 && begin <= end, "hgd_sample_pairwise: bad record range");
  HGD_REQUIRE(n_items >= 1 && n_items < (int64_t{1} << 32), "hgd_sample_pairwise: n_items");
  HGD_REQUIRE(n_negs >= 0, "hgd_sample_pairwise: n_negs < 0");
  if (begin == end) return HGD_OK;
  HGD_REQUIRE(order && rec_user && rec_item && user_rowptr && out_u && out_i &&
                  (out_j || n_negs == 0),
              "hgd_sample_pairwise: null pointer");
  Mt g{mt_state, mt_state[kMtN]};
  s = sample_cf("hgd_sample_pairwise", g, mt_state, order, begin, end, rec_user, rec_item,
                user_rowptr, user_items, n_users, n_items, n_negs, out_u, out_i, out_j);
  if (s != HGD_OK) return s;
  mt_state[kMtN] = g.index;
  return HGD_OK;
}

extern "C" hgd_status hgd_sample_unified(const hgd_unified_batch* b) {
  using namespace hgd;
  clear_error();
  HGD_REQUIRE(b, "hgd_sample_unified: null request");
  hgd_status s = check_state(b->py_state);
  if (s != HGD_OK) return s;
  s = check_state(b->np_state);
  if (s != HGD_OK) return s;
  HGD_REQUIRE(b->begin >= 0 && b->begin <= b->end, "hgd_sample_unified: bad record range");
  HGD_REQUIRE(b->n_items >= 1 && b->n_items < (int64_t{1} << 32), "hgd_sample_unified: n_items");
  HGD_REQUIRE(b->n_negs >= 0, "hgd_sample_unified: n_negs < 0");
  HGD_REQUIRE(b->batch_kg >= 0, "hgd_sample_unified: batch_kg < 0");
  // np.random.randint(0) raises; the 32-bit masked path below covers every table the int64
  // positions of one host can index in practice
  HGD_REQUIRE(b->n_sel >= 1 && b->n_sel <= (int64_t{1} << 32),
              "hgd_sample_unified: selected-triple table of %lld rows",
              static_cast<long long>(b->n_sel));
  HGD_REQUIRE(b->n_tails >= 1 && b->n_tails < (int64_t{1} << 32) && b->n_heads >= 1,
              "hgd_sample_unified: empty tail / head table");
  HGD_REQUIRE(b->begin == b->end || (b->order && b->rec_user && b->rec_item && b->user_rowptr &&
                                      b->out_u && b->out_i && (b->out_j || b->n_negs == 0)),
              "hgd_sample_unified: null CF pointer");
  HGD_REQUIRE(b->sel_head && b->sel_rel && b->sel_tail && b->all_tails && b->tail_rowptr &&
                  b->tail_sorted,
              "hgd_sample_unified: null KG table");
  HGD_REQUIRE(b->batch_kg == 0 || (b->out_h && b->out_r && b->out_t && b->out_n),
              "hgd_sample_unified: null KG output");
  // 1. the CF records and their negatives: Python's stream
  Mt py{b->py_state, b->py_state[kMtN]};
  s = sample_cf("hgd_sample_unified", py, b->py_state, b->order, b->begin, b->end, b->rec_user,
                b->rec_item, b->user_rowptr, b->user_items, b->n_users, b->n_items, b->n_negs,
                b->out_u, b->out_i, b->out_j);
  if (s != HGD_OK) return s;
  // 2. np.random.randint(n_sel, size=batch_kg): the legacy RandomState path
  //    (_rand_int64 -> _random_bounded_uint64_fill with use_masked): rng = n_sel - 1; rng == 0
  //    draws nothing; rng == 2^32 - 1 takes whole 32-bit outputs; otherwise 32-bit outputs are
  //    masked to rng's bit length and redrawn while above rng
  Mt np{b->np_state, b->np_state[kMtN]};
  const uint64_t rng = static_cast<uint64_t>(b->n_sel) - 1;
  uint32_t mask = static_cast<uint32_t>(rng);
  mask |= mask >> 1;
  mask |= mask >> 2;
  mask |= mask >> 4;
  mask |= mask >> 8;
  mask |= mask >> 16;
  for (int64_t k = 0; k < b->batch_kg; ++k) {
    uint64_t v = 0;
    if (rng == 0xffffffffull) {
      v = np.next();
    } else if (rng != 0) {
      do {
        v = np.next() & mask;
      } while (v > rng);
    }
    const int64_t hp = b->sel_head[v];
    if (hp < 0 || hp >= b->n_heads) {
      b->py_state[kMtN] = py.index;
      b->np_state[kMtN] = np.index;
      return fail(HGD_ERR_INVALID_ARG, "hgd_sample_unified: head position %lld out of range",
                  static_cast<long long>(hp));
    }
    b->out_h[k] = b->head_ids ? b->head_ids[hp] : hp;
    b->out_r[k] = b->sel_rel[v];
    b->out_t[k] = b->sel_tail[v];
    b->out_n[k] = hp;  // the head's position until step 3 replaces it
  }
  b->np_state[kMtN] = np.index;
  // 3. per selected head, random.choice(all_tails) redrawn while in the head's tail set
  for (int64_t k = 0; k < b->batch_kg; ++k) {
    const int64_t hp = b->out_n[k];
    const int64_t lo = b->tail_rowptr[hp], hi = b->tail_rowptr[hp + 1];
    if (hi - lo >= b->n_tails) {  // the reference would loop forever
      b->py_state[kMtN] = py.index;
      return fail(HGD_ERR_INVALID_ARG,
                  "hgd_sample_unified: the head at position %lld has every tail of the epoch",
                  static_cast<long long>(hp));
    }
    int64_t neg = b->all_tails[py.below(static_cast<uint64_t>(b->n_tails))];
    while (sorted_contains64(b->tail_sorted, lo, hi, neg))
      neg = b->all_tails[py.below(static_cast<uint64_t>(b->n_tails))];
    b->out_n[k] = neg;
  }
  b->py_state[kMtN] = py.index;
  return HGD_OK;
}
