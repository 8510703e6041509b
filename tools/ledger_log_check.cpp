// ledger_log_check.cpp — the transfer ledger's log commitment and log audit in
// host C++ (csrc/ledger_log.h: the 14-felt leaf, HostLog on acc_layout.h's host
// tree, the receipt check; csrc/ledger_audit.h: the audit's host path) under
// the sanitizers, against a brute-force scan of the log and a naive recursive
// tree, at 1, 2, 3, 5, 65 and 131 entries in a ledger of exactly that capacity,
// with double spends among the entries, committed in one step and in several,
// across a reserve; the receipt check with all 32 sibling slots in use; the
// shared receipt walk on its own under a ballot leaf and a ledger leaf; the
// audit of an exactly-full log, honest and tampered.  A stand-alone CPU
// program; device code runs under no sanitizer.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/ledger_log_check.cpp -o ledger_log_check && ./ledger_log_check
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/ballot_log.h"
#include "../qp-zk-circuits-rm_amd/csrc/ledger_audit.h"
#include "../qp-zk-circuits-rm_amd/csrc/ledger_log.h"

using namespace ql;

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

// the leaf by the definition: hash_no_pad of the 14 felts as a sponge that overwrites eight lanes per block
static Digest naive_leaf(const HostLedger &h, uint64_t s) {
  uint64_t in[LEAF_FELTS], st[12] = {0};
  for (int j = 0; j < 4; j++) in[j] = h.nullifier[s * 4 + j], in[5 + j] = h.amount[s * 4 + j], in[9 + j] = h.account[s * 4 + j];
  in[4] = h.number[s];
  in[13] = h.flags[s];
  for (uint32_t at = 0; at < LEAF_FELTS; at += 8) {
    for (uint32_t j = 0; j < 8 && at + j < LEAF_FELTS; j++) st[j] = in[at + j];
    ps::permute(st);
  }
  Digest d;
  memcpy(d.v, st, 32);
  return d;
}

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

static std::mt19937_64 rng(14);
static uint64_t felt() { return rng() % P; }

// every receipt of the committed log checks, and each tampering gives its reason
static void check_receipts(const HostLedger &h, const HostLog &log, const std::vector<Digest> &leaves) {
  const uint64_t n = log.n;
  CHECK(n == h.count());
  const Digest want = naive_root(leaves, n);
  CHECK(!memcmp(want.v, log.root(), 32));
  uint64_t root[4];
  memcpy(root, log.root(), 32);
  for (uint64_t seq = 0; seq < n; seq++) {
    uint64_t sib[ACC_PATH_SLOTS * 4], leaf[4], nul[4], acc[4];
    uint32_t bits, depth, amt[4];
    log.path(seq, sib, &bits, &depth, leaf);
    CHECK(!memcmp(leaf, leaves[seq].v, 32));
    memcpy(nul, &h.nullifier[seq * 4], 32);
    memcpy(acc, &h.account[seq * 4], 32);
    memcpy(amt, &h.amount[seq * 4], 16);
    const uint64_t num = h.number[seq];
    const uint8_t fl = h.flags[seq];
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_OK);
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl ^ FLAG_CREDITED, sib, bits, depth) == RECEIPT_ROOT);
    CHECK(receipt_check(root, n, seq, nul, num + 1, amt, acc, fl, sib, bits, depth) == RECEIPT_ROOT);
    CHECK(receipt_check(root, n, seq, nul, P, amt, acc, fl, sib, bits, depth) == RECEIPT_NON_CANONICAL);
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl | 2, sib, bits, depth) == RECEIPT_NON_CANONICAL);
    for (int j = 0; j < 4; j++) {
      amt[j] ^= 1;
      CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_ROOT);
      amt[j] ^= 1;
      acc[j] ^= 1;
      CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth) != RECEIPT_OK);
      acc[j] ^= 1;
    }
    acc[3] = P;
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_NON_CANONICAL);
    acc[3] = h.account[seq * 4 + 3];
    CHECK(receipt_check(root, n, n, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_SHAPE);
    CHECK(receipt_check(root, 0, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_SHAPE);
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth + 1) == RECEIPT_SHAPE);
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, ACC_PATH_SLOTS + 1) == RECEIPT_SHAPE);
    if (depth) {
      CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits ^ 1, depth) == RECEIPT_SHAPE);
      CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth - 1) == RECEIPT_SHAPE);
      sib[(depth - 1) * 4 + 3] ^= 1;
      CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_ROOT);
      sib[(depth - 1) * 4 + 3] ^= 1;
    }
    sib[depth * 4] = 1;  // depth <= 31 < ACC_PATH_SLOTS
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_SHAPE);
    sib[depth * 4] = P;
    CHECK(receipt_check(root, n, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_NON_CANONICAL);
    sib[depth * 4] = 0;
    if (seq == n - 1 && n > 1)  // one more leaf gives the last entry another shape
      CHECK(receipt_check(root, n + 1, seq, nul, num, amt, acc, fl, sib, bits, depth) == RECEIPT_SHAPE);
  }
}

// n entries (every third a double spend of an earlier one where there is one, five accounts, limbs at
// their edges) into a ledger of `capacity`
static void fill(HostLedger &h, uint64_t n) {
  uint64_t accounts[5][4];
  for (auto &a : accounts)
    for (uint64_t &x : a) x = felt();
  for (uint64_t i = h.count(); i < n; i++) {
    uint64_t nul[4] = {felt(), felt(), felt(), felt()}, first;
    if (i % 3 == 2) memcpy(nul, &h.nullifier[(rng() % i) * 4], 32);
    if (i % 5 == 1) nul[0] = (nul[0] & ~h.mask) | (h.mask - 1);  // crowd the table's end: chains that wrap
    uint32_t amt[4] = {(uint32_t)rng(), i % 4 ? (uint32_t)rng() : 0xFFFFFFFFu, (uint32_t)rng(), i % 7 ? (uint32_t)rng() : 0};
    h.admit(nul, 2 * i + 1, amt, accounts[i % 5], &first);
  }
}

static void run(uint64_t n, uint64_t capacity, const std::vector<uint64_t> &steps, uint64_t reserve_to) {
  HostLedger h;
  h.open(capacity);
  HostLog log;
  std::vector<Digest> leaves;
  for (uint64_t upto : steps) {
    fill(h, upto);
    CHECK(log.commit(h) && log.n == upto);
    for (uint64_t s = leaves.size(); s < upto; s++) {
      Digest d;
      log_leaf(&h.nullifier[s * 4], h.number[s], &h.amount[s * 4], &h.account[s * 4], h.flags[s], d.v);
      const Digest by_definition = naive_leaf(h, s);
      CHECK(!memcmp(d.v, by_definition.v, 32));
      leaves.push_back(d);
    }
    const Digest want = naive_root(leaves, upto);
    CHECK(!memcmp(want.v, log.root(), 32));
    CHECK(log.commit(h) && !memcmp(want.v, log.root(), 32));  // nothing new
    for (uint64_t m = 1; m <= upto; m++) {
      uint64_t got[4];
      log.prefix_root(m, log_node, got);
      const Digest at_m = naive_root(leaves, m);
      CHECK(!memcmp(got, at_m.v, 32));
    }
  }
  CHECK(log.n == n && leaves.size() == n);
  check_receipts(h, log, leaves);
  if (reserve_to) {
    uint64_t before[4];
    memcpy(before, log.root(), 32);
    h.reserve(reserve_to);
    log.drop();
    CHECK(log.commit(h) && log.capacity == reserve_to && !memcmp(before, log.root(), 32));
    check_receipts(h, log, leaves);
  }
}

// a receipt whose 32 sibling slots are all in use cannot come from a tree (the deepest path is 31): the
// checker reads all 32 slots and refuses the depth, for every n and seq
static void check_all_slots() {
  uint64_t sib[ACC_PATH_SLOTS * 4], root[4] = {1, 2, 3, 4}, nul[4] = {5, 6, 7, 8}, acc[4] = {9, 10, 11, 12};
  uint32_t amt[4] = {1, 2, 3, 4};
  for (uint64_t &x : sib) x = felt();
  for (uint64_t n : {(uint64_t)1, (uint64_t)2, qpk::ACC_MAX_LEAVES})
    for (uint64_t seq : {(uint64_t)0, n - 1}) {
      CHECK(receipt_check(root, n, seq, nul, 0, amt, acc, 1, sib, 0xFFFFFFFFu, 32) == RECEIPT_SHAPE);
      CHECK(receipt_check(root, n, seq, nul, 0, amt, acc, 1, sib, 0, 32) == RECEIPT_SHAPE);
    }
  // the deepest real shape, 31 siblings and a non-zero slot 31: refused for the slot, not read past it
  const uint64_t n = qpk::ACC_MAX_LEAVES, seq = n - 1;
  CHECK(receipt_check(root, n, seq, nul, 0, amt, acc, 1, sib, 0x7FFFFFFFu, 31) == RECEIPT_SHAPE);
  for (int j = 0; j < 4; j++) sib[31 * 4 + j] = 0;
  CHECK(receipt_check(root, n, seq, nul, 0, amt, acc, 1, sib, 0x7FFFFFFFu, 31) == RECEIPT_ROOT);
  sib[31 * 4 + 3] = P;
  CHECK(receipt_check(root, n, seq, nul, 0, amt, acc, 1, sib, 0x7FFFFFFFu, 31) == RECEIPT_NON_CANONICAL);
}

// acc_layout.h's receipt_walk on its own, under a ballot leaf and a ledger leaf, at the sizes that promote
// a node at each level, against HostTree's paths: every path walks to the root, and a flipped depth, a
// flipped side bit, a sibling above the depth and a sibling felt of p each give their reason
static void check_walk() {
  for (uint64_t n : {1ull, 2ull, 3ull, 5ull, 8ull, 9ull})
    for (int ballot = 0; ballot < 2; ballot++) {
      qpk::HostTree t;
      t.open(n);
      for (uint64_t seq = 0; seq < n; seq++) {
        const uint64_t nul[4] = {felt(), felt(), felt(), felt()}, acc[4] = {felt(), felt(), felt(), felt()};
        const uint32_t amt[4] = {(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng()};
        if (ballot)
          qb::log_leaf(nul, seq + 1, 3, t.node(0, seq));
        else
          log_leaf(nul, seq + 1, amt, acc, 1, t.node(0, seq));
      }
      t.append(n, log_node);
      for (uint64_t seq = 0; seq < n; seq++) {
        uint64_t sib[ACC_PATH_SLOTS * 4], leaf[4];
        uint32_t bits, depth;
        t.path(seq, sib, &bits, &depth, leaf);
        auto walk = [&](uint32_t b, uint32_t d) { return qpk::receipt_walk(t.root(), n, seq, leaf, sib, b, d, log_node); };
        CHECK(walk(bits, depth) == RECEIPT_OK);
        CHECK(walk(bits, depth ^ 1) == RECEIPT_SHAPE);
        CHECK(walk(bits ^ 1, depth) == RECEIPT_SHAPE);
        sib[depth * 4] = 1;
        CHECK(walk(bits, depth) == RECEIPT_SHAPE);
        sib[depth * 4] = 0;
        sib[1] = P;
        CHECK(walk(bits, depth) == RECEIPT_NON_CANONICAL);
      }
    }
}

// the host audit of an exactly-full log against a brute-force scan
static void check_audit(uint64_t n) {
  HostLedger h;
  h.open(n);
  fill(h, n);
  HostLog log;
  CHECK(log.commit(h));
  // brute force: the first entry of each nullifier is credited; per-account exact sums in first-credit order
  std::vector<uint64_t> pa, ps, pf;
  std::map<std::vector<uint64_t>, size_t> at;
  uint64_t credited = 0, tot[5] = {0, 0, 0, 0, 0};
  for (uint64_t s = 0; s < n; s++) {
    bool first = true;
    for (uint64_t e = 0; e < s; e++) first = first && memcmp(&h.nullifier[e * 4], &h.nullifier[s * 4], 32);
    CHECK(first == bool(h.flags[s] & FLAG_CREDITED));
    if (!first) continue;
    credited++;
    const std::vector<uint64_t> key(&h.account[s * 4], &h.account[s * 4] + 4);
    if (!at.count(key)) {
      at[key] = pf.size();
      pa.insert(pa.end(), key.begin(), key.end());
      ps.insert(ps.end(), 4, 0);
      pf.push_back(s);
    }
    for (int j = 0; j < 4; j++) ps[at[key] * 4 + j] += h.amount[s * 4 + j], tot[1 + j] += h.amount[s * 4 + j];
  }
  tot[0] = credited;
  AuditLog g;
  g.nullifiers = h.nullifier.data(), g.numbers = h.number.data(), g.amounts = h.amount.data();
  g.accounts = h.account.data(), g.flags = h.flags.data(), g.n = n;
  const uint64_t ms[2] = {1, n / 2 + 1};
  uint64_t croots[8];
  for (int i = 0; i < 2; i++) log.prefix_root(ms[i], log_node, croots + 4 * i);
  AuditClaims c;
  c.root = log.root(), c.totals = tot, c.pay_accounts = pa.data(), c.pay_sums = ps.data(), c.pay_first_seq = pf.data();
  c.npay = pf.size(), c.commit_roots = croots, c.commit_ns = ms, c.ncommit = 2;
  CHECK(audit_refusal(g, c).empty());
  AuditReport r;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_OK && r.witness == AUDIT_NONE && r.credited == credited && r.accounts == pf.size());
  CHECK(!memcmp(r.root, log.root(), 32) && !memcmp(r.sums, tot + 1, 32));
  // the same total split another way is the same claim; one unit more is not
  if (ps[3] >> 32) {
    ps[3] -= 1ull << 32, ps[2] += 1;
    audit_host(g, c, r);
    CHECK(r.status == AUDIT_OK);
  }
  ps[3] += 1;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_PAYOUTS && r.witness == 0);
  ps[3] -= 1;
  c.npay -= 1;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_PAYOUTS && r.witness == c.npay);
  c.npay += 1;
  tot[4] += 1;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_TOTALS);
  tot[4] -= 1;
  croots[4] ^= 1;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_COMMITMENT && r.witness == 1);
  croots[4] ^= 1;
  if (n > 2) {  // entry 2 is a double spend: flag it credited
    std::vector<uint8_t> fl(h.flags);
    CHECK(!(fl[2] & FLAG_CREDITED));
    fl[2] |= FLAG_CREDITED;
    g.flags = fl.data();
    audit_host(g, c, r);
    CHECK(r.status == AUDIT_CREDIT_RULE && r.witness == 2 && r.first < 2);
    fl[2] = 2;
    audit_host(g, c, r);
    CHECK(r.status == AUDIT_NON_CANONICAL && r.witness == 2 && !r.root[0] && !r.credited);
    g.flags = h.flags.data();
  }
  if (n > 1) {
    std::vector<uint64_t> num(h.number);
    num[n - 1] = num[n - 2];
    g.numbers = num.data();
    audit_host(g, c, r);
    CHECK(r.status == AUDIT_ORDER && r.witness == n - 1);
  }
}

// audit_common.h through ql::'s entry points, on a log of three credited transfers, against literals: a
// commitment naming n + 1, a wrong root at index 0 and at the last index, cast_count = the last number
void shared_commitments() {
  const uint64_t n = 3, nul[12] = {7, 0, 0, 0, 7, 0, 0, 1, 7, 0, 0, 2}, num[3] = {4, 6, 9};
  const uint64_t acc[12] = {1, 2, 3, 4, 1, 2, 3, 5, 1, 2, 3, 4};
  const uint32_t amt[12] = {0, 0, 0, 5, 0, 0, 0, 6, 0, 0, 1, 7};
  const uint8_t fl[3] = {1, 1, 1};
  AuditLog g;
  g.nullifiers = nul, g.numbers = num, g.amounts = amt, g.accounts = acc, g.flags = fl, g.n = n;
  HostLedger led;
  HostLog log;
  AuditFacts f;
  CHECK(audit_facts_host(g, AuditClaims(), led, log, f));
  uint64_t roots[12], ns[3] = {1, 2, 3};
  for (int i = 0; i < 3; i++) log.prefix_root(ns[i], log_node, roots + 4 * i);
  AuditClaims c;
  c.commit_roots = roots, c.commit_ns = ns, c.ncommit = 3;
  AuditReport r;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_OK && r.witness == AUDIT_NONE && r.witness == ~0ull);
  ns[1] = n + 1;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_COMMITMENT && r.witness == 1 && r.first == ~0ull);
  CHECK(audit_failure_text(r) == "the log fails its audit: earlier commitment does not hold (commitment 1)");
  ns[1] = 2;
  roots[3] ^= 1;
  roots[11] ^= 1;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_COMMITMENT && r.witness == 0);
  roots[3] ^= 1;
  audit_host(g, c, r);
  CHECK(r.status == AUDIT_COMMITMENT && r.witness == 2);
  ns[0] = 0;
  CHECK(audit_refusal(g, c) == "commitment 0 names n = 0");
  CHECK(restore_refusal(num, n, 8, 9) == "cast_count 9 is not above the log's last transfer number 9");
  CHECK(restore_refusal(num, n, 8, 10).empty());
  CHECK(restore_refusal(num, n, 2, 10) ==
        "capacity 2 for a log of 3 entries: it must hold them (and at least one) and be at most 2^31");
  CHECK(restore_refusal(num, MAX_CAPACITY + 1, 8, 10) == "a log of 2147483649 entries: a ledger holds at most 2^31");
}

int main() {
  shared_commitments();
  const uint64_t a[4] = {0, 0, 0, 1ull << 32}, b[4] = {0, 0, 1, 0}, c[4] = {0, ~0ull, ~0ull, ~0ull}, d[4] = {1, 0, 0, 0};
  const uint64_t c1[4] = {0, ~0ull, ~0ull, ~0ull - 1};
  CHECK(sums_equal(a, b) && !sums_equal(a, d) && sums_equal(c, c) && !sums_equal(c, d) && !sums_equal(c, c1));
  for (uint64_t n : {1ull, 2ull, 3ull, 5ull, 65ull, 131ull}) {
    run(n, n, {n}, 0);          // capacity-full, one commit
    run(n, 2 * n + 3, {n}, 0);  // room to spare: the reserved layout's offsets differ
    check_audit(n);
  }
  run(65, 65, {1, 2, 3, 64, 65}, 130);  // incremental over the fold bound, then a reserve
  run(64, 100, {7, 14, 63, 64}, 64);    // a reserve down to exactly full
  run(131, 131, {1, 100, 101, 130, 131}, 4096);
  check_all_slots();
  check_walk();
  check_audit(200);
  printf("ledger_log_check: ok\n");
  return 0;
}
