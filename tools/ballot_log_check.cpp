// ballot_log_check.cpp — the ballot box's log commitment in host C++
// (csrc/ballot_table.h: the read-only find; csrc/ballot_log.h: the leaf and node hashes, HostLog on
// acc_layout.h's host tree, path extraction, the receipt check) under the sanitizers, against a
// brute-force scan of the log and a naive recursive tree, at 1, 2, 3, 64 and 65
// entries and on a capacity-full box, with doubles among the entries, committed
// in one step and in several, across a reserve.  A stand-alone CPU program;
// device code runs under no sanitizer.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/ballot_log_check.cpp -o ballot_log_check && ./ballot_log_check
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/ballot_log.h"

using namespace qb;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

struct Digest {
  uint64_t v[4];
};

// node j of level l of the tree over leaves [0, n), by the convention's definition, from the leaves
static Digest naive_node(const std::vector<Digest> &leaves, uint64_t n, uint32_t l, uint64_t j) {
  if (!l) return leaves[j];
  const uint64_t below = (n + (1ull << (l - 1)) - 1) >> (l - 1);
  const Digest a = naive_node(leaves, n, l - 1, 2 * j);
  if (2 * j + 1 >= below) return a;
  const Digest b = naive_node(leaves, n, l - 1, 2 * j + 1);
  Digest o;
  log_node(a.v, b.v, o.v);
  return o;
}

static Digest naive_root(const std::vector<Digest> &leaves, uint64_t n) {
  uint32_t top = 0;
  while ((1ull << top) < n) top++;
  return naive_node(leaves, n, top, 0);
}

static uint64_t brute_find(const HostBox &b, const uint64_t q[4]) {
  for (uint64_t s = 0; s < b.count(); s++)
    if (!memcmp(&b.nullifier[s * 4], q, 32)) return s;  // the first admitted one is the counted one
  return NOT_FOUND;
}

static std::mt19937_64 rng(11);
static uint64_t felt() { return rng() % P; }

// every receipt of the committed log checks, and each tampering gives its reason
static void check_receipts(const HostBox &box, const HostLog &log, const std::vector<Digest> &leaves) {
  const uint64_t n = log.n;
  CHECK(n == box.count());
  const Digest want = naive_root(leaves, n);
  CHECK(!memcmp(want.v, log.root(), 32));
  uint64_t root[4];
  memcpy(root, log.root(), 32);
  for (uint64_t seq = 0; seq < n; seq++) {
    uint64_t sib[ACC_PATH_SLOTS * 4], leaf[4];
    uint32_t bits, depth;
    log.path(seq, sib, &bits, &depth, leaf);
    CHECK(!memcmp(leaf, leaves[seq].v, 32));
    const uint64_t *nul = &box.nullifier[seq * 4];
    const uint64_t num = box.number[seq];
    const uint8_t fl = box.flags[seq];
    CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits, depth) == RECEIPT_OK);
    CHECK(receipt_check(root, n, seq, nul, num, fl ^ FLAG_VOTE, sib, bits, depth) == RECEIPT_ROOT);
    CHECK(receipt_check(root, n, seq, nul, num, fl ^ FLAG_COUNTED, sib, bits, depth) == RECEIPT_ROOT);
    CHECK(receipt_check(root, n, seq, nul, num + 1, fl, sib, bits, depth) == RECEIPT_ROOT);
    CHECK(receipt_check(root, n, seq, nul, P, fl, sib, bits, depth) == RECEIPT_NON_CANONICAL);
    CHECK(receipt_check(root, n, seq, nul, num, fl | 4, sib, bits, depth) == RECEIPT_NON_CANONICAL);
    CHECK(receipt_check(root, n, n, nul, num, fl, sib, bits, depth) == RECEIPT_SHAPE);
    CHECK(receipt_check(root, 0, seq, nul, num, fl, sib, bits, depth) == RECEIPT_SHAPE);
    CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits, depth + 1) == RECEIPT_SHAPE);
    CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits, ACC_PATH_SLOTS + 1) == RECEIPT_SHAPE);
    if (depth) {
      CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits ^ 1, depth) == RECEIPT_SHAPE);
      CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits, depth - 1) == RECEIPT_SHAPE);
      sib[(depth - 1) * 4 + 3] ^= 1;
      CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits, depth) == RECEIPT_ROOT);
      sib[(depth - 1) * 4 + 3] ^= 1;
    }
    if (depth < ACC_PATH_SLOTS) {
      sib[depth * 4] = 1;
      CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits, depth) == RECEIPT_SHAPE);
      sib[depth * 4] = P;
      CHECK(receipt_check(root, n, seq, nul, num, fl, sib, bits, depth) == RECEIPT_NON_CANONICAL);
      sib[depth * 4] = 0;
    }
    if (seq == n - 1 && n > 1)  // one more leaf gives the last entry another shape
      CHECK(receipt_check(root, n + 1, seq, nul, num, fl, sib, bits, depth) == RECEIPT_SHAPE);
  }
}

// n entries (every third a double of an earlier one where there is one) into a box of `capacity`,
// the tree committed after each of `steps`, then a reserve to `reserve_to` (0: none)
static void run(uint64_t n, uint64_t capacity, const std::vector<uint64_t> &steps, uint64_t reserve_to) {
  HostBox box;
  box.open(capacity);
  HostLog log;
  std::vector<Digest> leaves;
  size_t next = 0;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t nul[4] = {felt(), felt(), felt(), felt()}, first;
    if (i % 3 == 2) memcpy(nul, &box.nullifier[(rng() % i) * 4], 32);
    if (i % 5 == 1) nul[0] = (nul[0] & ~box.mask) | (box.mask - 1);  // crowd the table's end: chains that wrap
    box.admit(nul, 2 * i + 1, i & 1, &first);
    if (next < steps.size() && steps[next] == i + 1) {
      next++;
      CHECK(log.commit(box) && log.n == i + 1);
      for (uint64_t s = leaves.size(); s <= i; s++) {
        Digest d;
        log_leaf(&box.nullifier[s * 4], box.number[s], box.flags[s], d.v);
        leaves.push_back(d);
      }
      const Digest want = naive_root(leaves, i + 1);
      CHECK(!memcmp(want.v, log.root(), 32));
      CHECK(log.commit(box));  // nothing new
      CHECK(!memcmp(want.v, log.root(), 32));
    }
  }
  CHECK(log.n == n && leaves.size() == n);
  check_receipts(box, log, leaves);
  // find: every entry's nullifier gives the counted entry; absent keys with a crowded, an empty and the last home slot
  for (uint64_t s = 0; s < n; s++) {
    const uint64_t got = box.find(&box.nullifier[s * 4]);
    CHECK(got == brute_find(box, &box.nullifier[s * 4]) && got <= s && (box.flags[got] & FLAG_COUNTED));
  }
  for (uint64_t home : {box.mask - 1, box.mask, (uint64_t)0, box.mask / 2}) {
    uint64_t q[4] = {(felt() & ~box.mask) | home, felt(), felt(), felt()};
    CHECK(box.find(q) == brute_find(box, q));
  }
  if (reserve_to) {
    uint64_t before[4];
    memcpy(before, log.root(), 32);
    box.reserve(reserve_to);
    log.drop();
    CHECK(log.commit(box) && log.capacity == reserve_to && !memcmp(before, log.root(), 32));
    check_receipts(box, log, leaves);
    for (uint64_t s = 0; s < n; s++) CHECK(box.find(&box.nullifier[s * 4]) == brute_find(box, &box.nullifier[s * 4]));
  }
}

int main() {
  // the shape rule against the level table
  for (uint64_t n : {1ull, 2ull, 3ull, 5ull, 64ull, 65ull, 131ull})
    for (uint64_t seq = 0; seq < n; seq++) {
      qpk::AccLevels lv;
      CHECK(qpk::acc_levels_reserved(n, n, lv));
      uint32_t m = 0;
      for (uint32_t l = 0; l + 1 < lv.nlevels; l++)
        if (((seq >> l) ^ 1) < lv.len[l]) m |= 1u << l;
      CHECK(qpk::path_levels(seq, n) == m);
    }
  CHECK(qpk::path_levels(0, qpk::ACC_MAX_LEAVES) == 0x7FFFFFFFu && qpk::path_levels(qpk::ACC_MAX_LEAVES - 1, qpk::ACC_MAX_LEAVES) == 0x7FFFFFFFu);
  for (uint64_t n : {1ull, 2ull, 3ull, 64ull, 65ull}) {
    run(n, n, {n}, 0);              // capacity-full, one commit
    run(n, 2 * n + 3, {n}, 0);      // room to spare: the reserved layout's offsets differ
  }
  run(65, 65, {1, 2, 3, 64, 65}, 130);  // incremental over the fold bound, then a reserve
  run(64, 100, {7, 14, 63, 64}, 64);    // a reserve down to exactly full
  run(200, 200, {1, 100, 101, 199, 200}, 4096);
  printf("ballot_log_check: ok\n");
  return 0;
}
