// claims_check.cpp — the payout claims commitment in host C++ (csrc/claims.h:
// the order, the five-limb total, the claim leaf, HostClaims on acc_layout.h's
// host tree, the checker) under the sanitizers: the host sort, the
// normalisation, the tree and every claim at A = 0, 1, 2, 3, 5, 65, 131 and 1025
// rows from logs with double spends between the credits and with m0 > 0,
// against a brute-force rank, 128-bit arithmetic and a naive recursive tree; a
// tamper of every word of an absence and of a membership claim; and the checker
// fed out-of-range pos, depth, bits, found and count, each of which must be
// refused (the count of those cases is printed).
// A stand-alone CPU program; device code runs under no sanitizer.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/claims_check.cpp -o claims_check && ./claims_check
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/claims.h"

using namespace qcl;

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
  claim_node(a.v, b.v, o.v);
  return o;
}

// one claim with its own storage, as the ABI lays it out
struct Claim {
  uint64_t x[4], pos;
  uint32_t found;
  uint64_t account[2][4], first_seq[2], sib[2][ACC_PATH_SLOTS * 4];
  uint32_t total[2][LIMBS], bits[2], depth[2];
  Slot slot(int i) const { return Slot{account[i], total[i], first_seq[i], sib[i], bits[i], depth[i]}; }
  int check(const uint64_t root[4], uint64_t count) const { return qcl::check(root, count, x, found, pos, slot(0), slot(1)); }
};

static Claim claim_of(const HostClaims &h, const uint64_t x[4]) {
  Claim p;
  memset(&p, 0, sizeof p);
  memcpy(p.x, x, 32);
  bool f;
  p.pos = h.search(x, &f);
  p.found = f;
  const bool has[2] = {!f && p.pos > 0, p.pos < h.count()};
  const uint64_t at[2] = {p.pos - 1, p.pos};
  for (int i = 0; i < 2; i++)
    if (has[i]) {
      memcpy(p.account[i], &h.accounts[at[i] * 4], 32);
      memcpy(p.total[i], &h.totals[at[i] * LIMBS], LIMBS * 4);
      p.first_seq[i] = h.first_seq[at[i]];
      h.tree.path(at[i], p.sib[i], &p.bits[i], &p.depth[i], nullptr);
    }
  return p;
}

typedef unsigned __int128 u128;
struct Wide {  // an exact total below 2^160: the high 32 bits and the low 128
  uint64_t hi;
  u128 lo;
  void add(u128 a) {
    const u128 s = lo + a;
    hi += s < lo;
    lo = s;
  }
  void limbs(uint32_t t[5]) const {
    t[0] = (uint32_t)hi;
    for (int i = 0; i < 4; i++) t[1 + i] = (uint32_t)(lo >> (96 - 32 * i));
  }
};

static std::mt19937_64 rng(20260101);
static uint64_t felt() { return rng() % P; }

// a log of n entries over `accounts` accounts, a third of them not credited; amounts of the named kind
struct Log {
  std::vector<uint64_t> account;
  std::vector<uint32_t> amount;
  std::vector<uint8_t> flags;
};
static Log make_log(uint64_t n, const std::vector<uint64_t> &keys, int kind) {
  Log g;
  const uint64_t a = keys.size() / 4;
  for (uint64_t seq = 0; seq < n; seq++) {
    const uint64_t who = seq < a ? seq : rng() % (a ? a : 1);  // every account once, then again at random
    for (int f = 0; f < 4; f++) g.account.push_back(a ? keys[who * 4 + f] : felt());
    for (int f = 0; f < 4; f++) g.amount.push_back(kind == 0 ? (uint32_t)rng() : kind == 1 ? 0xFFFFFFFFu : 0u);
    g.flags.push_back(a && (seq < a || rng() % 3) ? 1 : 0);
  }
  return g;
}

static void check_range(const Log &g, uint64_t m0, uint64_t m1, uint64_t want_rows, uint64_t *refused) {
  ql::RoundRows rows;
  ql::round_payouts_host(g.account.data(), g.amount.data(), g.flags.data(), m0, m1, rows);
  HostClaims h;
  h.build(rows);
  // brute force: exact totals and first_seq per account over the credited entries of the range
  struct Row {
    Wide t;
    uint64_t first;
  };
  std::map<std::vector<uint64_t>, Row> owed;
  Wide grand{0, 0};
  for (uint64_t seq = m0; seq < m1; seq++) {
    if (!(g.flags[seq] & 1)) continue;
    std::vector<uint64_t> k(&g.account[seq * 4], &g.account[seq * 4] + 4);
    auto it = owed.find(k);
    if (it == owed.end()) it = owed.insert({k, Row{{0, 0}, seq}}).first;
    u128 amt = 0;
    for (int f = 0; f < 4; f++) amt = amt << 32 | g.amount[seq * 4 + f];
    it->second.t.add(amt);
    grand.add(amt);
  }
  const uint64_t A = owed.size();
  CHECK(h.count() == A);
  if (want_rows != ~0ull) CHECK(A == want_rows);
  uint32_t t[5];
  grand.limbs(t);
  CHECK(!memcmp(t, h.total, sizeof t));
  std::vector<Digest> leaves(A);
  uint64_t j = 0;
  for (const auto &kv : owed) {  // std::map orders vectors of unsigned words as key_compare does
    CHECK(!memcmp(kv.first.data(), &h.accounts[j * 4], 32));
    CHECK(kv.second.first == h.first_seq[j]);
    kv.second.t.limbs(t);
    CHECK(!memcmp(t, &h.totals[j * LIMBS], sizeof t));
    claim_leaf(kv.first.data(), t, kv.second.first, leaves[j].v);
    CHECK(!memcmp(leaves[j].v, h.tree.node(0, j), 32));
    j++;
  }
  if (!A) {
    CHECK(!(h.root[0] | h.root[1] | h.root[2] | h.root[3]));
  } else {
    uint32_t top = 0;
    while ((1ull << top) < A) top++;
    const Digest r = naive_node(leaves, A, top, 0);
    CHECK(!memcmp(r.v, h.root, 32));
  }
  // claims: every member, below all, above all, and a successor of every member
  std::vector<std::vector<uint64_t>> qs = {{0, 0, 0, 0}, {P - 1, P - 1, P - 1, P - 1}};
  for (const auto &kv : owed) {
    qs.push_back(kv.first);
    std::vector<uint64_t> up = kv.first;
    if (up[3] < P - 1) up[3]++, qs.push_back(up);
  }
  for (const auto &x : qs) {
    const Claim p = claim_of(h, x.data());
    uint64_t rank = 0;
    for (const auto &kv : owed) rank += kv.first < x;
    CHECK(p.pos == rank && p.found == (owed.count(x) ? 1u : 0u));
    CHECK(p.check(h.root, A) == RECEIPT_OK);
    // out-of-range words: the checker refuses and reads nothing it should not
    Claim q = p;
    q.pos = A + 1 + rng() % 5;
    CHECK(q.check(h.root, A) == RECEIPT_SHAPE);
    q = p, q.pos = ~0ull;
    CHECK(q.check(h.root, A) == RECEIPT_SHAPE);
    for (uint32_t found : {2u, 3u, 0x80000000u, ~0u}) {
      q = p, q.found = found;
      CHECK(q.check(h.root, A) == RECEIPT_SHAPE);
      ++*refused;
    }
    for (int sl = 0; sl < 2; sl++) {
      q = p, q.depth[sl] = 33 + (uint32_t)(rng() % 1000);
      CHECK(q.check(h.root, A) == RECEIPT_SHAPE);
      q = p, q.depth[sl] = ~0u, q.bits[sl] = ~0u;
      CHECK(q.check(h.root, A) == RECEIPT_SHAPE);
    }
    CHECK(p.check(h.root, ACC_MAX_LEAVES + 1) == RECEIPT_SHAPE);
    CHECK(p.check(h.root, ~0ull) == RECEIPT_SHAPE);
    if (A) CHECK(p.check(h.root, 0) != RECEIPT_OK);
    *refused += 8 + (A != 0);
  }
}

static void tamper_table() {
  std::vector<uint64_t> keys;
  for (int i = 0; i < 21 * 4; i++) keys.push_back(felt());
  const Log g = make_log(40, keys, 0);
  ql::RoundRows rows;
  ql::round_payouts_host(g.account.data(), g.amount.data(), g.flags.data(), 0, 40, rows);
  HostClaims h;
  h.build(rows);
  CHECK(h.count() == 21);
  uint64_t member[4], absent[4];
  memcpy(member, &h.accounts[20 * 4], 32);
  memcpy(absent, &h.accounts[19 * 4], 32);
  absent[3] = absent[3] < P - 1 ? absent[3] + 1 : absent[3] - 1;
  uint64_t refused = 0, tried = 0;
  for (const uint64_t *x : {member, absent}) {
    const Claim p = claim_of(h, x);
    CHECK(p.check(h.root, 21) == RECEIPT_OK);
    // every 64-bit and 32-bit word of the slots the claim uses, the root, found, pos and count
    for (int sl = 0; sl < 2; sl++) {
      if (sl == 0 && (p.found || !p.pos)) continue;
      for (int f = 0; f < 4; f++) {
        Claim q = p;
        q.account[sl][f] ^= 1;
        tried++, refused += q.check(h.root, 21) != RECEIPT_OK;
      }
      for (uint32_t f = 0; f < LIMBS; f++) {
        Claim q = p;
        q.total[sl][f] ^= 1;
        tried++, refused += q.check(h.root, 21) != RECEIPT_OK;
      }
      Claim q = p;
      q.first_seq[sl] ^= 1;
      tried++, refused += q.check(h.root, 21) != RECEIPT_OK;
      for (uint32_t w = 0; w < p.depth[sl] * 4; w++) {
        q = p, q.sib[sl][w] ^= 1;
        tried++, refused += q.check(h.root, 21) != RECEIPT_OK;
      }
      q = p, q.sib[sl][p.depth[sl] * 4] = 1;  // a non-zero slot above the depth
      tried++, refused += q.check(h.root, 21) == RECEIPT_SHAPE;
      q = p, q.bits[sl] ^= 1;
      tried++, refused += q.check(h.root, 21) == RECEIPT_SHAPE;
      q = p, q.depth[sl]--;
      tried++, refused += q.check(h.root, 21) == RECEIPT_SHAPE;
    }
    for (int f = 0; f < 4; f++) {
      uint64_t r[4];
      memcpy(r, h.root, 32);
      r[f] ^= 1;
      tried++, refused += p.check(r, 21) != RECEIPT_OK;
    }
    Claim q = p;
    q.found ^= 1;
    tried++, refused += q.check(h.root, 21) != RECEIPT_OK;
    q = p, q.pos++;
    tried++, refused += q.check(h.root, 21) != RECEIPT_OK;
    q = p, q.pos--;
    tried++, refused += q.check(h.root, 21) != RECEIPT_OK;
    tried += 2, refused += (p.check(h.root, 20) != RECEIPT_OK) + (p.check(h.root, 22) != RECEIPT_OK);
    q = p, q.x[0] = P;
    tried++, refused += q.check(h.root, 21) == RECEIPT_NON_CANONICAL;
    q = p, q.first_seq[1] = P;
    tried++, refused += q.check(h.root, 21) == RECEIPT_NON_CANONICAL;
  }
  CHECK(refused == tried);
  printf("tamper table: %llu of %llu refused\n", (unsigned long long)refused, (unsigned long long)tried);
}

static void normalise_edges() {
  uint32_t t[5];
  const uint64_t top = ((uint64_t)1 << 31) * 0xFFFFFFFFull;  // 2^31 entries of limbs 0xFFFFFFFF
  const uint64_t all[4] = {top, top, top, top};
  normalise(all, t);
  Wide w{0, 0};
  w.hi = top >> 32;  // top << 96 passes 2^128: its high part, then the low 128 bits (the shift drops the rest)
  for (int i = 0; i < 4; i++) w.add((u128)top << (96 - 32 * i));
  uint32_t want[5];
  w.limbs(want);
  CHECK(!memcmp(t, want, sizeof t));
  const uint64_t zero[4] = {0, 0, 0, 0};
  normalise(zero, t);
  for (uint32_t v : t) CHECK(!v);
  const uint64_t three[4] = {3 * 0xFFFFFFFFull, 3 * 0xFFFFFFFFull, 3 * 0xFFFFFFFFull, 3 * 0xFFFFFFFFull};
  normalise(three, t);  // 3 (2^128 - 1)
  const uint32_t w3[5] = {2, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFDu};
  CHECK(!memcmp(t, w3, sizeof t));
}

int main() {
  normalise_edges();
  uint64_t refused = 0;
  for (uint64_t A : {0ull, 1ull, 2ull, 3ull, 5ull, 65ull, 131ull, 1025ull})
    for (int kind = 0; kind < 3; kind++) {
      std::vector<uint64_t> keys;
      for (uint64_t i = 0; i < A * 4; i++) keys.push_back(kind == 2 ? (i % 4 == 3 ? i : 7) : felt());  // kind 2: felt 3 alone differs
      const uint64_t n = A * 2 + 9;
      const Log g = make_log(n, keys, kind);
      check_range(g, 0, n, A, &refused);
      check_range(g, A / 2 + 1, n - 2, ~0ull, &refused);  // m0 > 0: accounts credited before and inside
      check_range(g, 3, 3, 0, &refused);
    }
  // a range whose entries are all double spends
  Log g = make_log(30, std::vector<uint64_t>(40, 5), 0);
  for (uint64_t seq = 10; seq < 30; seq++) g.flags[seq] = 0;
  check_range(g, 10, 30, 0, &refused);
  tamper_table();
  printf("claims_check ok: %llu out-of-range claims refused\n", (unsigned long long)refused);
  return 0;
}
