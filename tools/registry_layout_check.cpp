// registry_layout_check.cpp — the voter registry's host-only arithmetic
// (csrc/registry_layout.h) under the sanitizers: the capacity layout table,
// the dirty ranges of an append and the sort / duplicate check of a replace
// batch, from 0 to 2^31 voters and at both edges of the capacity.  A
// stand-alone CPU program; device code runs under no sanitizer.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/registry_layout_check.cpp -o registry_layout_check && ./registry_layout_check
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <set>
#include "../qp-zk-circuits-rm_amd/csrc/registry_layout.h"

using namespace qpk;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static uint64_t ceil_shift(uint64_t n, uint32_t l) { return (n + (((uint64_t)1 << l) - 1)) >> l; }

// the table of n voters in a capacity layout: lengths, offsets, no level reaching into the next
static void check_table(uint64_t n, uint64_t cap) {
  RegistryLevels lv;
  CHECK(registry_levels_reserved(n, cap, lv));
  const uint64_t reserved = registry_reserved(cap);
  uint32_t caplevels = 0;
  for (uint64_t len = cap;; len = (len + 1) / 2) {
    caplevels++;
    if (len == 1) break;
  }
  CHECK(caplevels <= REG_MAX_LEVELS && lv.nlevels <= caplevels);
  CHECK((n == 0) == (lv.nlevels == 0));
  uint64_t o = 0;
  for (uint32_t l = 0; l < caplevels; l++) {
    CHECK(lv.off[l] == o);
    o += ceil_shift(cap, l);
    if (l < lv.nlevels) {
      CHECK(lv.len[l] == ceil_shift(n, l));
      CHECK(lv.off[l] + lv.len[l] <= o);  // inside the level's reservation
    }
  }
  CHECK(o == reserved);
  if (n) CHECK(lv.len[lv.nlevels - 1] == 1 && (lv.nlevels == 1 || lv.len[lv.nlevels - 2] == 2));
  if (n == cap) {  // the keyed layout
    CHECK(lv.total() == reserved);
  }
}

// an append n_old -> n_new: per level one range that holds every changed node and stays inside the level
static void check_append(uint64_t n_old, uint64_t n_new) {
  RegistryRange rg[REG_MAX_LEVELS];
  const uint32_t nl = registry_append_ranges(n_old, n_new, rg);
  RegistryLevels lv;
  CHECK(registry_levels_reserved(n_new, n_new, lv) && lv.nlevels == nl);
  for (uint32_t l = 0; l < nl; l++) {
    CHECK(rg[l].end == lv.len[l] && rg[l].first < rg[l].end);
    CHECK(rg[l].first == n_old >> l);
    // nodes below first cover only old leaves: node j spans leaves [j 2^l, (j + 1) 2^l)
    CHECK((rg[l].first << l) <= n_old);
    // the node that holds old leaf n_old - 1 and new leaf n_old (if one does) is in the range
    if (l) CHECK(2 * rg[l].first <= rg[l - 1].first + 1 && 2 * rg[l].first >= rg[l - 1].first - (rg[l - 1].first & 1));
    if (l) CHECK(2 * rg[l].first < lv.len[l - 1]);  // its source pair starts inside the level below
  }
}

int main() {
  // layout: sizes 0 .. 2^31, capacities at both edges (n, n + 1, 2 n, 2^31)
  const uint64_t M = REG_MAX_VOTERS;
  std::vector<uint64_t> sizes = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, M - 1, M};
  for (uint32_t b = 3; b <= 31; b++)
    for (int d = -1; d <= 1; d++) sizes.push_back(((uint64_t)1 << b) + d);
  for (uint64_t n : sizes) {
    if (n > M) continue;
    for (uint64_t cap : {n, n + 1, 2 * n, n + 1000, M - 1, M}) {
      if (cap < 1 || cap > M || cap < n) continue;
      check_table(n, cap);
    }
  }
  RegistryLevels lv;
  CHECK(!registry_levels_reserved(0, 0, lv) && !registry_levels_reserved(2, 1, lv));
  CHECK(!registry_levels_reserved(1, M + 1, lv) && registry_reserved(M + 1) == 0 && registry_reserved(0) == 0);
  CHECK(registry_reserved(1) == 1 && registry_reserved(2) == 3 && registry_reserved(5) == 5 + 3 + 2 + 1);
  CHECK(registry_reserved(M) == 2 * M - 1);
  for (uint64_t n = 0; n <= 300; n++)
    for (uint64_t cap = n ? n : 1; cap <= 310; cap++) check_table(n, cap);
  // append ranges: every small pair, and the edges up to 2^31
  for (uint64_t a = 0; a <= 130; a++)
    for (uint64_t b = a + 1; b <= 140; b++) check_append(a, b);
  for (uint64_t a : sizes)
    for (uint64_t b : sizes)
      if (a < b && b <= M) check_append(a, b);
  // the dirty ranges against a brute-force tree over leaf generations (small sizes)
  for (uint64_t a = 0; a <= 40; a++)
    for (uint64_t b = a + 1; b <= 45; b++) {
      RegistryRange rg[REG_MAX_LEVELS];
      const uint32_t nl = registry_append_ranges(a, b, rg);
      // node j of level l changes iff it covers a leaf >= a, or the tree of a voters had no such node
      for (uint32_t l = 0; l < nl; l++)
        for (uint64_t j = 0; j < ceil_shift(b, l); j++) {
          const bool existed = j < ceil_shift(a, l), covers_new = ((j + 1) << l) > a;
          const bool changed = !existed || covers_new;
          if (changed) CHECK(j >= rg[l].first && j < rg[l].end);
        }
    }
  // replace batches: order, bounds, duplicates
  std::mt19937_64 rng(7);
  for (uint32_t k : {0u, 1u, 2u, 17u, 1000u, 8193u}) {
    for (uint64_t n : {(uint64_t)k + 1, (uint64_t)1 << 20, M}) {
      if (n < k) continue;
      std::set<uint64_t> s;
      while (s.size() < k) s.insert(rng() % n);
      std::vector<uint64_t> idx(s.begin(), s.end());
      std::shuffle(idx.begin(), idx.end(), rng);
      std::vector<uint32_t> order;
      uint32_t bad = ~0u;
      CHECK(registry_replace_order(idx.data(), k, n, order, &bad) && order.size() == k);
      for (uint32_t b = 1; b < k; b++) CHECK(idx[order[b - 1]] < idx[order[b]]);
      if (k >= 2) {
        std::vector<uint64_t> dup = idx;
        dup[k - 1] = dup[0];
        CHECK(!registry_replace_order(dup.data(), k, n, order, &bad) && bad == k - 1);
        dup = idx;
        dup[k / 2] = n;  // out of range wins over the order
        CHECK(!registry_replace_order(dup.data(), k, n, order, &bad) && bad == k / 2);
        dup[k / 2] = ~(uint64_t)0;
        CHECK(!registry_replace_order(dup.data(), k, n, order, &bad) && bad == k / 2);
      }
    }
  }
  printf("registry layout check ok\n");
  return 0;
}
