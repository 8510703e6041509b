// acc_layout_check.cpp — the accumulator tree's host-only half
// (csrc/acc_layout.h) under the sanitizers: the capacity layout table, the
// dirty ranges of an append and the sort / duplicate check of a replace batch,
// from 0 to 2^31 leaves and at both edges of the capacity; the shape rule of a
// path; and the host tree (HostTree) against a naive recursive tree, its paths
// walked back to the root, under a toy node hash.  A stand-alone CPU program;
// device code runs under no sanitizer.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/acc_layout_check.cpp -o acc_layout_check && ./acc_layout_check
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <set>
#include "../qp-zk-circuits-rm_amd/csrc/acc_layout.h"

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
  AccLevels lv;
  CHECK(acc_levels_reserved(n, cap, lv));
  const uint64_t reserved = acc_reserved(cap);
  uint32_t caplevels = 0;
  for (uint64_t len = cap;; len = (len + 1) / 2) {
    caplevels++;
    if (len == 1) break;
  }
  CHECK(caplevels <= ACC_MAX_LEVELS && lv.nlevels <= caplevels);
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
  AccRange rg[ACC_MAX_LEVELS];
  const uint32_t nl = acc_append_ranges(n_old, n_new, rg);
  AccLevels lv;
  CHECK(acc_levels_reserved(n_new, n_new, lv) && lv.nlevels == nl);
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

struct Digest {
  uint64_t v[4];
};

// a node hash for the host tree's checks: not a hash to rely on, only one under which left and
// right, and every felt, matter (HostTree is generic in it; the real one is ballot_log.h's log_node)
static void toy_node(const uint64_t l[4], const uint64_t r[4], uint64_t out[4]) {
  uint64_t t[4];
  for (int k = 0; k < 4; k++)
    t[k] = (l[k] * 0x9E3779B97F4A7C15ull + 1) ^ ((r[(k + 1) & 3] + k) * 0xC2B2AE3D27D4EB4Full) ^ (l[(k + 3) & 3] >> 7);
  memcpy(out, t, 32);
}

// node j of level l of the tree over leaves [0, n), by the convention's definition, from the leaves
static Digest naive_node(const std::vector<Digest> &leaves, uint64_t n, uint32_t l, uint64_t j) {
  if (!l) return leaves[j];
  const Digest a = naive_node(leaves, n, l - 1, 2 * j);
  if (2 * j + 1 >= ceil_shift(n, l - 1)) return a;
  const Digest b = naive_node(leaves, n, l - 1, 2 * j + 1);
  Digest o;
  toy_node(a.v, b.v, o.v);
  return o;
}

// a HostTree of `cap` grown to each size of `steps` (ascending, sizes already reached are skipped):
// after each step every node equals the naive tree's, and every path leads from its leaf to the root
static void check_host_tree(uint64_t n, uint64_t cap, const std::vector<uint64_t> &steps) {
  std::mt19937_64 rng(n * 1000003 + cap);
  std::vector<Digest> leaves(n);
  for (Digest &d : leaves)
    for (uint64_t &x : d.v) x = rng();
  HostTree t;
  t.open(cap);
  CHECK(t.capacity == cap && t.n == 0 && t.dig.size() == acc_reserved(cap) * 4);
  for (uint64_t to : steps) {
    if (to <= t.n) continue;
    for (uint64_t i = t.n; i < to; i++) memcpy(t.node(0, i), leaves[i].v, 32);
    t.append(to, toy_node);
    CHECK(t.n == to && t.lv.len[0] == to);
    for (uint32_t l = 0; l < t.lv.nlevels; l++)
      for (uint64_t j = 0; j < t.lv.len[l]; j++) {
        const Digest want = naive_node(leaves, to, l, j);
        CHECK(!memcmp(want.v, t.node(l, j), 32));
      }
    for (uint64_t i = 0; i < to; i++) {
      uint64_t sib[ACC_PATH_SLOTS * 4], leaf[4], cur[4];
      uint32_t bits = ~0u, depth = ~0u;
      t.path(i, sib, &bits, &depth, leaf);
      CHECK(!memcmp(leaf, leaves[i].v, 32));
      const uint32_t m = path_levels(i, to);
      CHECK(depth == (uint32_t)__builtin_popcount(m) && depth < ACC_PATH_SLOTS && !(bits >> depth));
      for (uint32_t k = depth * 4; k < ACC_PATH_SLOTS * 4; k++) CHECK(sib[k] == 0);
      memcpy(cur, leaf, 32);
      uint32_t d = 0;
      for (uint32_t l = 0; l < 32; l++) {
        if (!(m >> l & 1)) continue;
        CHECK((bits >> d & 1) == ((i >> l) & 1));
        if (bits >> d & 1)
          toy_node(sib + d * 4, cur, cur);
        else
          toy_node(cur, sib + d * 4, cur);
        d++;
      }
      CHECK(!memcmp(cur, t.root(), 32));
    }
    uint64_t sib[ACC_PATH_SLOTS * 4];
    uint32_t bits, depth;
    t.path(to - 1, sib, &bits, &depth, nullptr);  // the leaf digest is optional
  }
  t.drop();
  CHECK(t.capacity == 0 && t.n == 0 && t.dig.empty());
}

int main() {
  // layout: sizes 0 .. 2^31, capacities at both edges (n, n + 1, 2 n, 2^31)
  const uint64_t M = ACC_MAX_LEAVES;
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
  AccLevels lv;
  CHECK(!acc_levels_reserved(0, 0, lv) && !acc_levels_reserved(2, 1, lv));
  CHECK(!acc_levels_reserved(1, M + 1, lv) && acc_reserved(M + 1) == 0 && acc_reserved(0) == 0);
  CHECK(acc_reserved(1) == 1 && acc_reserved(2) == 3 && acc_reserved(5) == 5 + 3 + 2 + 1);
  CHECK(acc_reserved(M) == 2 * M - 1);
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
      AccRange rg[ACC_MAX_LEVELS];
      const uint32_t nl = acc_append_ranges(a, b, rg);
      // node j of level l changes iff it covers a leaf >= a, or the tree of a voters had no such node
      for (uint32_t l = 0; l < nl; l++)
        for (uint64_t j = 0; j < ceil_shift(b, l); j++) {
          const bool existed = j < ceil_shift(a, l), covers_new = ((j + 1) << l) > a;
          const bool changed = !existed || covers_new;
          if (changed) CHECK(j >= rg[l].first && j < rg[l].end);
        }
    }
  // the shape rule against the level table, and at the largest tree
  for (uint64_t n : {1ull, 2ull, 3ull, 5ull, 64ull, 65ull, 131ull})
    for (uint64_t i = 0; i < n; i++) {
      CHECK(acc_levels_reserved(n, n, lv));
      uint32_t m = 0;
      for (uint32_t l = 0; l + 1 < lv.nlevels; l++)
        if (((i >> l) ^ 1) < lv.len[l]) m |= 1u << l;
      CHECK(path_levels(i, n) == m);
    }
  CHECK(path_levels(0, M) == 0x7FFFFFFFu && path_levels(M - 1, M) == 0x7FFFFFFFu && path_levels(0, 1) == 0);
  // the host tree with a toy node hash: grown in one step and in several, full and with room to spare
  for (uint64_t n : {1ull, 2ull, 3ull, 64ull, 65ull, 129ull, 200ull})
    for (uint64_t cap : {n, 2 * n + 3}) {
      check_host_tree(n, cap, {n});
      check_host_tree(n, cap, {1, n / 2, n / 2 + 1, n - 1, n});
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
  printf("acc_layout_check: ok\n");
  return 0;
}
