// nullifier_set_check.cpp — the nullifier-set commitment in host C++
// (csrc/nullifier_set.h: the order, the set leaf, HostSet on acc_layout.h's host
// tree, the checker) under the sanitizers: the host sort, the tree and every
// proof at m = 0, 1, 2, 3, 5, 65, 131 and 1025 members with non-members between
// them, against a brute-force rank and a naive recursive tree; the tamper table
// (every word of an absence and of a membership proof); duplicates; and the
// checker fed out-of-range pos, depth, bits, found and m, whose refusals it
// counts.  A stand-alone CPU program; device code runs under no sanitizer.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/nullifier_set_check.cpp -o nullifier_set_check && ./nullifier_set_check
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/nullifier_set.h"

using namespace qns;

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
  set_node(a.v, b.v, o.v);
  return o;
}

// one proof with its own storage, as the ABI lays it out
struct Proof {
  uint64_t x[4], pos;
  uint32_t found;
  uint64_t key[2][4], seq[2], sib[2][ACC_PATH_SLOTS * 4];
  uint32_t bits[2], depth[2];
  Slot slot(int i) const { return Slot{key[i], seq[i], sib[i], bits[i], depth[i]}; }
  int check(const uint64_t root[4], uint64_t m) const { return qns::check(root, m, x, found, pos, slot(0), slot(1)); }
};

static Proof prove(const HostSet &s, const uint64_t x[4]) {
  Proof p;
  memset(&p, 0, sizeof p);
  memcpy(p.x, x, 32);
  bool f;
  p.pos = s.search(x, &f);
  p.found = f;
  const bool has[2] = {!f && p.pos > 0, p.pos < s.m()};
  const uint64_t at[2] = {p.pos - 1, p.pos};
  for (int i = 0; i < 2; i++)
    if (has[i]) {
      memcpy(p.key[i], &s.keys[at[i] * 4], 32);
      p.seq[i] = s.seqs[at[i]];
      s.tree.path(at[i], p.sib[i], &p.bits[i], &p.depth[i], nullptr);
    }
  return p;
}

static uint64_t refusals = 0;
static void refused(const Proof &p, const uint64_t root[4], uint64_t m) {
  CHECK(p.check(root, m) != RECEIPT_OK);
  refusals++;
}

// every word of p changed alone (the key's words only where told: an absence proof holds for every key
// between its leaves); the words of a slot the proof does not use are set, which the checker refuses too
static void tamper_table(const Proof &p, const uint64_t root[4], uint64_t m, bool key_too) {
  CHECK(p.check(root, m) == RECEIPT_OK);
  for (int i = 0; i < 4; i++) {
    uint64_t r[4];
    memcpy(r, root, 32);
    r[i] ^= 1;
    refused(p, r, m);
    if (key_too) {
      Proof t = p;
      t.x[i] ^= 1;
      refused(t, root, m);
    }
  }
  for (int s = 0; s < 2; s++) {
    for (int i = 0; i < 4; i++) {
      Proof t = p;
      t.key[s][i] ^= 1;
      refused(t, root, m);
    }
    for (uint32_t i = 0; i < ACC_PATH_SLOTS * 4; i++) {
      Proof t = p;
      t.sib[s][i] ^= 1;
      refused(t, root, m);
    }
    for (uint32_t b = 0; b < 32; b++) {
      Proof t = p;
      t.bits[s] ^= 1u << b;
      refused(t, root, m);
    }
    Proof t = p;
    t.seq[s] ^= 1;
    refused(t, root, m);
    for (uint32_t d : {0u, 1u, 31u, 32u, 33u, 0xFFFFFFFFu}) {
      if (d == p.depth[s]) continue;
      t = p;
      t.depth[s] = d;  // out of range too: the checker never indexes by a depth it has not matched to (j, m)
      refused(t, root, m);
    }
  }
  for (uint64_t pos : {p.pos - 1, p.pos + 1, m, m + 1, (uint64_t)1 << 31, (uint64_t)1 << 32, ~(uint64_t)0}) {
    if (pos == p.pos) continue;
    Proof t = p;
    t.pos = pos;
    refused(t, root, m);
  }
  for (uint32_t f : {1u - p.found, 2u, 0xFFFFFFFFu}) {
    Proof t = p;
    t.found = f;
    refused(t, root, m);
  }
  for (uint64_t mm : {((uint64_t)1 << 31) + 1, (uint64_t)1 << 40, ~(uint64_t)0}) refused(p, root, mm);
}

static void run_size(uint64_t m, std::mt19937_64 &rng) {
  const uint64_t n = 2 * m + 3;
  std::vector<uint64_t> nul(n * 4);
  std::vector<uint8_t> flags(n, 0);
  for (auto &v : nul) v = rng() % P;
  for (uint64_t i = 0, left = m; i < n && left; i++)
    if (n - i == left || rng() % 2) flags[i] = 2, left--;
  HostSet s;
  s.build(nul.data(), flags.data(), n, 2);
  CHECK(s.m() == m && s.dup == NOT_FOUND);
  std::vector<Digest> leaves(m);
  for (uint64_t j = 0; j < m; j++) {
    CHECK(flags[s.seqs[j]] && !memcmp(&s.keys[j * 4], &nul[(size_t)s.seqs[j] * 4], 32));
    if (j) CHECK(rec_less(&s.keys[(j - 1) * 4], s.seqs[j - 1], &s.keys[j * 4], s.seqs[j]));
    set_leaf(&s.keys[j * 4], s.seqs[j], leaves[j].v);
  }
  uint32_t top = 0;
  while (((m + (1ull << top) - 1) >> top) > 1) top++;
  const Digest zero{{0, 0, 0, 0}};
  const Digest want = m ? naive_node(leaves, m, top, 0) : zero;
  CHECK(!memcmp(want.v, s.root, 32));
  // every member, a key beside every member, the two ends
  std::vector<uint64_t> q;
  for (uint64_t j = 0; j < m; j++) {
    q.insert(q.end(), &s.keys[j * 4], &s.keys[j * 4] + 4);
    uint64_t k[4];
    memcpy(k, &s.keys[j * 4], 32);
    k[3] = k[3] + 1 < P ? k[3] + 1 : k[3] - 1;
    q.insert(q.end(), k, k + 4);
  }
  const uint64_t ends[8] = {0, 0, 0, 0, P - 1, P - 1, P - 1, P - 1};
  q.insert(q.end(), ends, ends + 8);
  for (size_t i = 0; i < q.size() / 4; i++) {
    const uint64_t *x = &q[i * 4];
    uint64_t rank = 0;
    bool in = false;
    for (uint64_t j = 0; j < m; j++) {
      rank += key_compare(&s.keys[j * 4], x) < 0;
      in = in || key_equal(&s.keys[j * 4], x);
    }
    const Proof p = prove(s, x);
    CHECK(p.pos == rank && (p.found != 0) == in);
    CHECK(p.check(s.root, m) == RECEIPT_OK);
  }
  if (m >= 3) {
    uint64_t k[4];
    memcpy(k, &s.keys[(m / 2) * 4], 32);
    tamper_table(prove(s, k), s.root, m, true);  // membership
    k[3] = k[3] + 1 < P ? k[3] + 1 : k[3] - 1;
    const Proof a = prove(s, k);
    if (!a.found) tamper_table(a, s.root, m, false);  // absence between two leaves
    tamper_table(prove(s, ends), s.root, m, false);
    tamper_table(prove(s, ends + 4), s.root, m, false);
    // an absence proof for a member cannot be assembled from honest leaves
    Proof t = prove(s, &s.keys[(m / 2) * 4]);
    for (uint64_t pos : {m / 2, m / 2 + 1}) {
      Proof f = t;
      f.found = 0;
      f.pos = pos;
      for (int i = 0; i < 2; i++) {
        const uint64_t at = pos - 1 + i;
        memset(f.sib[i], 0, sizeof f.sib[i]);
        memcpy(f.key[i], &s.keys[at * 4], 32);
        f.seq[i] = s.seqs[at];
        s.tree.path(at, f.sib[i], &f.bits[i], &f.depth[i], nullptr);
      }
      CHECK(f.check(s.root, m) == SET_ORDER);
      refusals++;
    }
  }
  printf("m = %llu of n = %llu: root, order, %zu proofs ok\n", (unsigned long long)m, (unsigned long long)n, q.size() / 4);
}

int main() {
  std::mt19937_64 rng(20260521);
  for (uint64_t m : {0, 1, 2, 3, 5, 65, 131, 1025}) run_size(m, rng);
  // the empty set: every absence holds with no path, under the zero root only
  {
    const uint64_t zero[4] = {0, 0, 0, 0}, one[4] = {1, 0, 0, 0}, x[4] = {5, 6, 7, 8};
    HostSet s;
    s.build(nullptr, nullptr, 0, 1);
    Proof p = prove(s, x);
    CHECK(p.check(zero, 0) == RECEIPT_OK && p.check(one, 0) == RECEIPT_ROOT);
    p.pos = 1;
    CHECK(p.check(zero, 0) == RECEIPT_SHAPE);
  }
  // duplicate members: the lowest offending seq
  {
    std::vector<uint64_t> nul(50 * 4);
    for (auto &v : nul) v = rng() % P;
    memcpy(&nul[44 * 4], &nul[7 * 4], 32);
    memcpy(&nul[41 * 4], &nul[30 * 4], 32);
    memcpy(&nul[47 * 4], &nul[7 * 4], 32);
    std::vector<uint8_t> flags(50, 1);
    HostSet s;
    s.build(nul.data(), flags.data(), 50, 1);
    CHECK(s.m() == 50 && s.dup == 41);
    flags[41] = 0;
    s.build(nul.data(), flags.data(), 50, 1);
    CHECK(s.m() == 49 && s.dup == 44);
  }
  printf("nullifier_set_check ok: %llu tampered or out-of-range proofs refused\n", (unsigned long long)refusals);
  return 0;
}
