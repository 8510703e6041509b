// ledger_restore_check.cpp — reopening a transfer ledger from its published log
// and payout rounds in host C++ (csrc/ledger_audit.h: the audit's passes over
// the new ledger's own buffers, restore_refusal, restore_verdict;
// csrc/ledger_rounds.h: round_payouts_host and its refusals) under the
// sanitizers, against a brute-force quadratic scan, at logs of 1, 2, 255, 256,
// 257 and 513 entries with runs of double spends, restored at exactly-full
// capacity and at 2 n + 3, every refusal, and every range of a small log plus
// the block-edge ranges of the large ones.  A stand-alone CPU program; device
// code, and anything loaded into Python, runs under no sanitizer.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/ledger_restore_check.cpp -o ledger_restore_check && ./ledger_restore_check
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/ledger_audit.h"
#include "../qp-zk-circuits-rm_amd/csrc/ledger_rounds.h"

using namespace ql;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static std::mt19937_64 rng(15);
static uint64_t felt() { return rng() % P; }

// n entries into h (every third a double spend of an earlier one, runs of them across 250..262, five
// accounts, limbs at their edges, chains that wrap the tables' end)
static void fill(HostLedger &h, uint64_t n) {
  uint64_t accounts[5][4];
  for (auto &a : accounts)
    for (uint64_t &x : a) x = felt();
  for (uint64_t i = h.count(); i < n; i++) {
    uint64_t nul[4] = {felt(), felt(), felt(), felt()}, first;
    const bool run = i >= 250 && i < 263;
    if (i % 3 == 2 || run) memcpy(nul, &h.nullifier[(rng() % i) * 4], 32);
    if (i % 5 == 1 && !run) nul[0] = (nul[0] & ~h.mask) | (h.mask - 1);
    uint32_t amt[4] = {(uint32_t)rng(), i % 4 ? (uint32_t)rng() : 0xFFFFFFFFu, (uint32_t)rng(), i % 7 ? (uint32_t)rng() : 0};
    h.admit(nul, 2 * i + 1, amt, accounts[i % 5], &first);
  }
}

static AuditLog log_of(const HostLedger &h) {
  AuditLog g;
  g.nullifiers = h.nullifier.data(), g.numbers = h.number.data(), g.amounts = h.amount.data();
  g.accounts = h.account.data(), g.flags = h.flags.data(), g.n = h.count();
  return g;
}

// brute force: the rows of [m0, m1) by a quadratic scan of the range
static RoundRows naive_round(const AuditLog &g, uint64_t m0, uint64_t m1) {
  RoundRows r;
  for (uint64_t s = m0; s < m1; s++) {
    if (!(g.flags[s] & FLAG_CREDITED)) continue;
    bool first = true;
    for (uint64_t e = m0; e < s; e++)
      first = first && !((g.flags[e] & FLAG_CREDITED) && !memcmp(g.accounts + e * 4, g.accounts + s * 4, 32));
    if (!first) continue;
    uint64_t sums[4] = {0, 0, 0, 0};
    for (uint64_t e = s; e < m1; e++)
      if ((g.flags[e] & FLAG_CREDITED) && !memcmp(g.accounts + e * 4, g.accounts + s * 4, 32))
        for (int j = 0; j < 4; j++) sums[j] += g.amounts[e * 4 + j];
    r.accounts.insert(r.accounts.end(), g.accounts + s * 4, g.accounts + s * 4 + 4);
    r.sums.insert(r.sums.end(), sums, sums + 4);
    r.first_seq.push_back(s);
  }
  return r;
}

static bool same_rows(const RoundRows &a, const RoundRows &b) {
  return a.accounts == b.accounts && a.sums == b.sums && a.first_seq == b.first_seq;
}

static void check_round(const AuditLog &g, uint64_t m0, uint64_t m1) {
  RoundRows got;
  round_payouts_host(g.accounts, g.amounts, g.flags, m0, m1, got);
  CHECK(same_rows(got, naive_round(g, m0, m1)));
  // the store: a sizing call, a short buffer, a full one
  uint64_t count = 77;
  round_store(got, 0, nullptr, nullptr, nullptr, &count);
  CHECK(count == got.count());
  const uint64_t cap = got.count() / 2 + 1;
  std::vector<uint64_t> a(cap * 4, 0xA5), s(cap * 4, 0xA5), f(cap, 0xA5);
  round_store(got, cap, a.data(), s.data(), f.data(), &count);
  const uint64_t k = got.count() < cap ? got.count() : cap;
  CHECK(count == got.count());
  if (k) CHECK(!memcmp(a.data(), got.accounts.data(), k * 32) && !memcmp(f.data(), got.first_seq.data(), k * 8));
  for (uint64_t i = k; i < cap; i++) CHECK(f[i] == 0xA5);
}

// the restored ledger against the one that published the log, then one more transfer and a double spend
static void check_restore(const HostLedger &h, uint64_t capacity) {
  const AuditLog g = log_of(h);
  const uint64_t n = g.n, cast_count = 2 * n + 7;
  CHECK(restore_refusal(g.numbers, n, capacity, cast_count).empty());
  HostLedger led;
  HostLog unused, log;
  AuditFacts f;
  AuditReport r;
  CHECK(audit_facts_host(g, AuditClaims(), led, unused, f, capacity, false));
  restore_verdict(f, n, nullptr, r);
  CHECK(r.status == AUDIT_OK && led.capacity == capacity && led.mask + 1 == table_slots(capacity));
  CHECK(led.count() == n && led.credited == h.credited && led.payee == h.payee);
  // brute force: the owner of every nullifier, every account's sums
  for (uint64_t s = 0; s < n; s++) {
    uint64_t owner = s;
    for (uint64_t e = 0; e < s && owner == s; e++)
      if (!memcmp(&h.nullifier[e * 4], &h.nullifier[s * 4], 32)) owner = e;
    CHECK(led.find(&h.nullifier[s * 4]) == owner && bool(led.flags[s] & FLAG_CREDITED) == (owner == s));
  }
  const RoundRows all = naive_round(g, 0, n);
  CHECK(all.count() == led.accounts());
  for (uint64_t i = 0; i < all.count(); i++) {
    uint64_t sums[4];
    CHECK(led.total_for(&all.accounts[i * 4], sums) && !memcmp(sums, &all.sums[i * 4], 32));
    CHECK(led.payee[i] == all.first_seq[i]);
  }
  // the root: the restored ledger's own commit equals the publisher's, whatever the two capacities
  HostLog published;
  CHECK(published.commit(h) && log.commit(led) && log.capacity == capacity && !memcmp(log.root(), published.root(), 32));
  memcpy(f.root, log.root(), 32);
  restore_verdict(f, n, published.root(), r);
  CHECK(r.status == AUDIT_OK);
  uint64_t other[4];
  memcpy(other, published.root(), 32);
  other[1] ^= 1;
  restore_verdict(f, n, other, r);
  CHECK(r.status == AUDIT_ROOT && audit_failure_text(r) == "the log fails its audit: claimed root differs");
  // it is an ordinary ledger: exactly full refuses by the caller's count; after a reserve it admits
  if (led.count() == led.capacity) led.reserve(capacity + 2);
  uint64_t nul[4] = {felt(), felt(), felt(), felt()}, acc[4] = {1, 2, 3, 4}, first = 0;
  uint32_t amt[4] = {1, 2, 3, 4};
  CHECK(led.admit(nul, cast_count, amt, acc, &first) && first == cast_count);
  CHECK(!led.admit(&h.nullifier[(n - 1) * 4], cast_count + 1, amt, acc, &first));
  CHECK(first == h.number[h.find(&h.nullifier[(n - 1) * 4])]);
  CHECK(log.commit(led) && log.n == n + 2);
}

static void check_refusals(const HostLedger &h) {
  const AuditLog g = log_of(h);
  const uint64_t n = g.n;
  CHECK(!restore_refusal(g.numbers, n, n - 1, 2 * n).empty() && !restore_refusal(g.numbers, n, 0, 2 * n).empty());
  CHECK(!restore_refusal(g.numbers, n, MAX_CAPACITY + 1, 2 * n).empty());
  CHECK(!restore_refusal(g.numbers, n, n, g.numbers[n - 1]).empty() && restore_refusal(g.numbers, n, n, g.numbers[n - 1] + 1).empty());
  CHECK(restore_refusal(nullptr, 0, 1, 0).empty() && !restore_refusal(nullptr, 0, 0, 0).empty());
  HostLedger led;
  HostLog unused;
  AuditFacts f;
  AuditReport r;
  auto verdict = [&](const AuditLog &bad) {
    if (!audit_facts_host(bad, AuditClaims(), led, unused, f, n + 3, false)) {
      audit_non_canonical(f.non_canonical, r);
      return;
    }
    restore_verdict(f, n, nullptr, r);
  };
  std::vector<uint8_t> fl(h.flags);
  std::vector<uint64_t> num(h.number), acc(h.account), nul(h.nullifier);
  AuditLog bad = g;
  // a credited double spend (entry 2 doubles an earlier one), and the lowest of two offenders
  CHECK(!(fl[2] & FLAG_CREDITED) && !(fl[n - 1] & FLAG_CREDITED));
  fl[n - 1] = 1, bad.flags = fl.data();
  verdict(bad);
  CHECK(r.status == AUDIT_CREDIT_RULE && r.witness == n - 1 && r.first < n - 1);
  fl[2] = 1;
  verdict(bad);
  CHECK(r.status == AUDIT_CREDIT_RULE && r.witness == 2 && r.first < 2);
  CHECK(audit_failure_text(r) == "the log fails its audit: credit rule broken (entry 2, its nullifier first at entry " +
                                     std::to_string(r.first) + ")");
  // a first entry left uncredited
  fl = h.flags, fl[0] = 0;
  verdict(bad);
  CHECK(r.status == AUDIT_CREDIT_RULE && r.witness == 0 && r.first == 0);
  // order, before the credit rule; non-canonical before both
  num[n - 1] = num[n - 2], bad.numbers = num.data();
  verdict(bad);
  CHECK(r.status == AUDIT_ORDER && r.witness == n - 1);
  acc[(n - 2) * 4 + 3] = P, bad.accounts = acc.data();
  verdict(bad);
  CHECK(r.status == AUDIT_NON_CANONICAL && r.witness == n - 2);
  nul[4] = P, bad.nullifiers = nul.data();
  verdict(bad);
  CHECK(r.status == AUDIT_NON_CANONICAL && r.witness == 1);
  CHECK(audit_failure_text(r) == "the log fails its audit: non-canonical entry (entry 1)");
  fl = h.flags, fl[1] = 2;
  bad = g, bad.flags = fl.data();
  verdict(bad);
  CHECK(r.status == AUDIT_NON_CANONICAL && r.witness == 1);
  verdict(g);  // a following good restore works
  CHECK(r.status == AUDIT_OK && led.count() == n && led.capacity == n + 3);
  // the rounds' refusals
  uint64_t count = 0, buf[4];
  CHECK(round_refusal(n, 0, n, 0, nullptr, nullptr, nullptr, &count).empty());
  CHECK(!round_refusal(n, 0, n, 0, nullptr, nullptr, nullptr, nullptr).empty());
  CHECK(!round_refusal(n, 2, 1, 0, nullptr, nullptr, nullptr, &count).empty());
  CHECK(!round_refusal(n, 0, n + 1, 0, nullptr, nullptr, nullptr, &count).empty());
  CHECK(!round_refusal(n, 0, n, 1, buf, buf, nullptr, &count).empty() && round_refusal(n, n, n, 1, buf, buf, buf, &count).empty());
  CHECK(round_log_refusal(g.accounts, g.flags, 0, n).empty());
  CHECK(!round_log_refusal(acc.data(), g.flags, 0, n).empty() && round_log_refusal(acc.data(), g.flags, 0, n - 2).empty());
  CHECK(!round_log_refusal(g.accounts, fl.data(), 1, 2).empty() && round_log_refusal(g.accounts, fl.data(), 2, n).empty());
}

int main() {
  for (uint64_t n : {1ull, 2ull, 255ull, 256ull, 257ull, 513ull}) {
    HostLedger h;
    h.open(n);
    fill(h, n);
    check_restore(h, n);          // exactly full
    check_restore(h, 2 * n + 3);  // room to spare: other table sizes, another tree layout
    const AuditLog g = log_of(h);
    for (uint64_t m0 : {0ull, 7ull, 255ull, 256ull, 257ull})
      for (uint64_t m1 : {(unsigned long long)m0, (unsigned long long)m0 + 1, 300ull, 513ull})
        if (m0 <= m1 && m1 <= n) check_round(g, m0, m1);
    check_round(g, 0, n);
    if (n == 513) {
      check_round(g, 250, 263);  // double spends only
      RoundRows none;
      round_payouts_host(g.accounts, g.amounts, g.flags, 250, 263, none);
      CHECK(none.count() == 0);
      check_refusals(h);
    }
  }
  {  // every range of a small log
    HostLedger h;
    h.open(24);
    fill(h, 24);
    const AuditLog g = log_of(h);
    for (uint64_t m0 = 0; m0 <= 24; m0++)
      for (uint64_t m1 = m0; m1 <= 24; m1++) check_round(g, m0, m1);
  }
  {  // 4096 entries of 2^128 - 1 to one account, split at 1000: the limb sums are exact
    const uint64_t n = 4096, cut = 1000;
    HostLedger h;
    h.open(n);
    uint64_t acc[4] = {9, 8, 7, 6}, first;
    uint32_t amt[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint64_t i = 0; i < n; i++) {
      uint64_t nul[4] = {felt(), felt(), felt(), felt()};
      CHECK(h.admit(nul, i, amt, acc, &first));
    }
    const AuditLog g = log_of(h);
    RoundRows a, b;
    round_payouts_host(g.accounts, g.amounts, g.flags, 0, cut, a);
    round_payouts_host(g.accounts, g.amounts, g.flags, cut, n, b);
    CHECK(a.count() == 1 && b.count() == 1 && a.first_seq[0] == 0 && b.first_seq[0] == cut);
    for (int j = 0; j < 4; j++) CHECK(a.sums[j] == cut * 0xFFFFFFFFull && b.sums[j] == (n - cut) * 0xFFFFFFFFull);
  }
  printf("ledger_restore_check: ok\n");
  return 0;
}
