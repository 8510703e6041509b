// ballot_audit_check.cpp — the host path of the log audit (csrc/ballot_audit.h:
// the screen, the count rule through HostBox's probe, the verdict; acc_layout.h's
// HostTree::prefix_root; the restore's checks) under the sanitizers, against
// brute force: a quadratic scan for the count rule and a naive recursive tree
// per m for the prefix roots.  Sizes 1, 2, 3, 5, 64, 65, 131, 257; every reason,
// each with its lowest witness.  A stand-alone CPU program; nothing loaded into
// Python runs under a sanitizer, and device code runs under none.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/ballot_audit_check.cpp -o ballot_audit_check && ./ballot_audit_check
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/ballot_audit.h"

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

struct Log {
  std::vector<uint64_t> nul, num;
  std::vector<uint8_t> fl;
  uint64_t n() const { return num.size(); }
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

static Digest naive_root(const Log &g, uint64_t m) {
  std::vector<Digest> leaves(m);
  for (uint64_t s = 0; s < m; s++) log_leaf(&g.nul[s * 4], g.num[s], g.fl[s], leaves[s].v);
  uint32_t top = 0;
  while ((1ull << top) < m) top++;
  return naive_node(leaves, m, top, 0);
}

// the audit by brute force: the definitions read off one by one
static AuditReport brute(const Log &g, const AuditClaims &c) {
  const uint64_t n = g.n();
  AuditReport r{AUDIT_OK, 0, AUDIT_NONE, AUDIT_NONE, {0, 0, 0, 0}, 0, 0, 0};
  for (uint64_t s = 0; s < n; s++) {
    bool bad = g.num[s] >= P || g.fl[s] > 3;
    for (int j = 0; j < 4; j++) bad |= g.nul[s * 4 + j] >= P;
    if (bad) {
      r.status = AUDIT_NON_CANONICAL;
      r.witness = s;
      return r;
    }
  }
  const Digest root = naive_root(g, n);
  memcpy(r.root, root.v, 32);
  for (uint64_t s = 0; s < n; s++)
    if (g.fl[s] & FLAG_COUNTED) {
      r.counted++;
      (g.fl[s] & FLAG_VOTE ? r.yes : r.no)++;
    }
  for (uint64_t s = 1; s < n; s++)
    if (g.num[s] <= g.num[s - 1]) {
      r.status = AUDIT_ORDER;
      r.witness = s;
      return r;
    }
  for (uint64_t s = 0; s < n; s++) {
    uint64_t first = s;
    for (uint64_t t = 0; t < s; t++)
      if (!memcmp(&g.nul[t * 4], &g.nul[s * 4], 32)) {
        first = t;
        break;
      }
    if (bool(g.fl[s] & FLAG_COUNTED) != (first == s)) {
      r.status = AUDIT_COUNT_RULE;
      r.witness = s;
      r.first = first;
      return r;
    }
  }
  if (c.tally && (c.tally[0] != r.yes || c.tally[1] != r.no)) {
    r.status = AUDIT_TALLY;
    return r;
  }
  if (c.root && memcmp(c.root, r.root, 32)) {
    r.status = AUDIT_ROOT;
    return r;
  }
  for (uint32_t i = 0; i < c.ncommit; i++) {
    bool holds = c.commit_ns[i] <= n;
    if (holds) {
      const Digest d = naive_root(g, c.commit_ns[i]);
      holds = !memcmp(d.v, c.commit_roots + (size_t)i * 4, 32);
    }
    if (!holds) {
      r.status = AUDIT_COMMITMENT;
      r.witness = i;
      return r;
    }
  }
  return r;
}

static std::mt19937_64 rng(23);
static uint64_t felt() { return rng() % P; }

// an honest log of n entries through a HostBox: every third a double of an earlier one where there is one,
// chains crowded at the table's end, numbers with gaps (rejected ballots take a number and no entry)
static Log honest(uint64_t n, HostBox &box) {
  box = HostBox();
  box.open(n);
  uint64_t number = 0;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t nul[4] = {felt(), felt(), felt(), felt()}, first;
    if (i % 3 == 2) memcpy(nul, &box.nullifier[(rng() % i) * 4], 32);
    if (i % 5 == 1) nul[0] = (nul[0] & ~box.mask) | (box.mask - 1);
    number += 1 + rng() % 3;
    box.admit(nul, number, rng() & 1, &first);
  }
  return Log{box.nullifier, box.number, box.flags};
}

static void audit_both(const Log &g, const AuditClaims &c, uint32_t status, uint64_t witness) {
  AuditReport got;
  const Log before = g;
  audit_host(g.nul.data(), g.num.data(), g.fl.data(), g.n(), c, AUDIT_ALL_REASONS, got);
  CHECK(before.nul == g.nul && before.num == g.num && before.fl == g.fl);
  const AuditReport want = brute(g, c);
  CHECK(want.status == status && want.witness == witness);
  CHECK(got.status == want.status && got.witness == want.witness && got.first == want.first);
  CHECK(!memcmp(got.root, want.root, 32) && got.yes == want.yes && got.no == want.no && got.counted == want.counted);
}

static void run(uint64_t n) {
  HostBox box;
  const Log g = honest(n, box);
  // the prefix roots of every m against a naive tree per m, in a tree laid out for n and in a roomier one
  std::vector<uint64_t> roots(n * 4);
  for (uint64_t cap : {n, 2 * n + 3}) {
    HostBox b2;
    HostLog log;
    AuditFacts f;
    CHECK(audit_facts_host(g.nul.data(), g.num.data(), g.fl.data(), n, cap, true, b2, log, f));
    CHECK(b2.slot.size() == table_slots(cap) && b2.count() == n && b2.yes == box.yes && b2.no == box.no);
    for (uint64_t s = 0; s < n; s++) CHECK(b2.find(&g.nul[s * 4]) == box.find(&g.nul[s * 4]));
    HostLog grown;  // the same leaves appended one at a time into a tree with room to spare
    grown.open(cap);
    for (uint64_t m = 1; m <= n; m++) {
      log_leaf(&g.nul[(m - 1) * 4], g.num[m - 1], g.fl[m - 1], grown.node(0, m - 1));
      grown.append(m, log_node);
      const Digest want = naive_root(g, m);
      uint64_t got[4];
      log.prefix_root(m, log_node, got);
      CHECK(!memcmp(got, want.v, 32) && !memcmp(grown.root(), want.v, 32));
      memcpy(&roots[(m - 1) * 4], got, 32);
    }
    for (uint64_t m = 1; m <= n; m++) {
      uint64_t got[4];
      grown.prefix_root(m, log_node, got);
      CHECK(!memcmp(got, &roots[(m - 1) * 4], 32));
    }
    CHECK(!memcmp(f.root, &roots[(n - 1) * 4], 32));
  }
  // the honest log with every claim; commitments at 1, the middle and n
  const uint64_t tally[2] = {box.yes, box.no};
  std::vector<uint64_t> cn = {1, n / 2 + 1, n}, cr;
  for (uint64_t m : cn) cr.insert(cr.end(), &roots[(m - 1) * 4], &roots[(m - 1) * 4] + 4);
  AuditClaims c;
  c.root = &roots[(n - 1) * 4];
  c.tally = tally;
  c.commit_roots = cr.data();
  c.commit_ns = cn.data();
  c.ncommit = 3;
  audit_both(g, c, AUDIT_OK, AUDIT_NONE);
  CHECK(audit_refusal(n, c).empty() && restore_refusal(g.num.data(), n, n, g.num[n - 1] + 1).empty());
  CHECK(!restore_refusal(g.num.data(), n, n, g.num[n - 1]).empty() && !restore_refusal(g.num.data(), n, n - 1, ~0ull).empty());
  CHECK(!audit_refusal(0, c).empty() && !audit_refusal(MAX_CAPACITY + 1, c).empty());
  // every reason, each tampering at the last entry and (two offenders: the lower is the witness) at an early one too
  const uint64_t hi = n - 1, lo = n > 4 ? 1 : hi;
  for (int what = 0; what < 3; what++) {
    Log t = g;
    for (uint64_t s : {hi, lo}) {
      if (what == 0) t.nul[s * 4 + 3] = P;
      if (what == 1) t.num[s] = ~0ull;
      if (what == 2) t.fl[s] = 4;
    }
    audit_both(t, c, AUDIT_NON_CANONICAL, lo);
  }
  if (n >= 2) {
    Log t = g;
    t.num[hi] = t.num[hi - 1];
    if (lo != hi) std::swap(t.num[lo], t.num[lo + 1]);
    audit_both(t, c, AUDIT_ORDER, lo != hi ? lo + 1 : hi);
    t.nul[3] = P;  // an earlier reason at a later place in the table's order still wins
    audit_both(t, c, AUDIT_NON_CANONICAL, 0);
  }
  {
    Log t = g;  // the counted bit flipped: on a first ballot it is cleared, on a double it is set
    t.fl[hi] ^= FLAG_COUNTED;
    if (lo != hi) t.fl[lo] ^= FLAG_COUNTED;
    audit_both(t, c, AUDIT_COUNT_RULE, lo);
    Log u = g;
    u.fl[0] ^= FLAG_VOTE;  // entry 0 is always counted
    audit_both(u, c, AUDIT_TALLY, AUDIT_NONE);
    AuditClaims c2 = c;
    c2.tally = nullptr;
    audit_both(u, c2, AUDIT_ROOT, AUDIT_NONE);
    c2.root = nullptr;
    audit_both(u, c2, AUDIT_COMMITMENT, 0);
    std::vector<uint64_t> cn2 = {1, n + 1, n};
    c2 = c;
    c2.commit_ns = cn2.data();
    audit_both(g, c2, AUDIT_COMMITMENT, 1);
    // restore's reasons: the tally and the commitments are not its business
    AuditReport r;
    audit_host(u.nul.data(), u.num.data(), u.fl.data(), n, c, AUDIT_RESTORE_REASONS, r);
    CHECK(r.status == AUDIT_ROOT && !audit_failure_text(r).empty());
    audit_host(g.nul.data(), g.num.data(), g.fl.data(), n, c2, AUDIT_RESTORE_REASONS, r);
    CHECK(r.status == AUDIT_OK);
    audit_host(t.nul.data(), t.num.data(), t.fl.data(), n, c, AUDIT_RESTORE_REASONS, r);
    CHECK(r.status == AUDIT_COUNT_RULE && audit_failure_text(r).find("entry " + std::to_string(lo)) != std::string::npos);
  }
  if (n > 8) {  // history rewritten below the middle commitment, the final root recomputed by the cheat
    Log t = g;
    uint64_t s = 2;  // a double's vote bit: the tally stays
    while (s < n / 2 && (t.fl[s] & FLAG_COUNTED)) s++;
    CHECK(s < n / 2);
    t.fl[s] ^= FLAG_VOTE;
    const Digest cheat = naive_root(t, n);
    AuditClaims c2 = c;
    c2.root = cheat.v;
    audit_both(t, c2, AUDIT_COMMITMENT, 1);
  }
}

// audit_common.h through qb::'s entry points, on a log of three first ballots, against literals: a
// commitment naming n + 1, a wrong root at index 0 and at the last index, cast_count = the last number
void shared_commitments() {
  const uint64_t n = 3, nul[12] = {7, 0, 0, 0, 7, 0, 0, 1, 7, 0, 0, 2}, num[3] = {4, 6, 9};
  const uint8_t fl[3] = {3, 2, 3};
  HostBox box;
  HostLog log;
  AuditFacts f;
  CHECK(audit_facts_host(nul, num, fl, n, n, true, box, log, f));
  uint64_t roots[12], ns[3] = {1, 2, 3};
  for (int i = 0; i < 3; i++) log.prefix_root(ns[i], log_node, roots + 4 * i);
  AuditClaims c;
  c.commit_roots = roots, c.commit_ns = ns, c.ncommit = 3;
  AuditReport r;
  audit_host(nul, num, fl, n, c, AUDIT_ALL_REASONS, r);
  CHECK(r.status == AUDIT_OK && r.witness == AUDIT_NONE && r.witness == ~0ull);
  ns[1] = n + 1;
  audit_host(nul, num, fl, n, c, AUDIT_ALL_REASONS, r);
  CHECK(r.status == AUDIT_COMMITMENT && r.witness == 1 && r.first == ~0ull);
  CHECK(audit_failure_text(r) == "the log fails its audit: an earlier commitment does not hold (commitment 1)");
  ns[1] = 2;
  roots[3] ^= 1;
  roots[11] ^= 1;
  audit_host(nul, num, fl, n, c, AUDIT_ALL_REASONS, r);
  CHECK(r.status == AUDIT_COMMITMENT && r.witness == 0);
  roots[3] ^= 1;
  audit_host(nul, num, fl, n, c, AUDIT_ALL_REASONS, r);
  CHECK(r.status == AUDIT_COMMITMENT && r.witness == 2);
  ns[0] = 0;
  CHECK(audit_refusal(n, c) == "commitment 0 names n = 0");
  CHECK(restore_refusal(num, n, 8, 9) == "cast_count 9 is not above the log's last ballot number 9");
  CHECK(restore_refusal(num, n, 8, 10).empty());
  CHECK(restore_refusal(num, n, 2, 10) ==
        "capacity 2 for a log of 3 entries: it must hold them (and at least one) and be at most 2^31");
  CHECK(restore_refusal(num, MAX_CAPACITY + 1, 8, 10) == "a log of 2147483649 entries: a box holds at most 2^31");
}

int main() {
  shared_commitments();
  for (uint64_t n : {1ull, 2ull, 3ull, 5ull, 64ull, 65ull, 131ull, 257ull}) run(n);
  printf("ballot_audit_check: ok\n");
  return 0;
}
