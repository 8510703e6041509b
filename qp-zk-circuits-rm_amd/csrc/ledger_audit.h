// ledger_audit.h — the audit of a published transfer log in host C++: the
// eight statuses and their witnesses, the verdict both paths share, and the host
// path itself (HostLedger's probes give the owner of a nullifier, the account
// sums and the payees; HostLog the root and the prefix roots).  Plain C++ next
// to ledger_log.h (no HIP); the commitment claims, a restore's refusals and the
// text of a failing audit are audit_common.h's, shared with the ballot log.
// Included by ledger_audit.cpp, by ledger.cpp
// (qp_ledger_restore runs reasons 1-3 and the root on the ledger it builds) and
// by the stand-alone checks tools/ledger_log_check.cpp and
// tools/ledger_restore_check.cpp.
//
// Definitions (DESIGN §14 and qpgpu.h state the same):
//   A published log is what qp_ledger_entries returns: nullifiers[n][4],
//   numbers[n], amounts[n][4] (32-bit limbs), accounts[n][4], flags[n], 1 <= n
//   <= 2^31.  Beside it come optional claims: a root, totals (credited and the
//   four limb sums over the credited entries), the payouts (accounts, limb sums,
//   first_seq, in first-credit order) and earlier commitments (root_i, n_i).
//   The audit reports the first reason that fires, in this order, with the
//   lowest offender as its witness, so the report is a function of the input:
//     OK            nothing below
//     NON_CANONICAL a nullifier or account felt >= p, a number >= p or flags >
//                   1; witness = the lowest such seq.  Nothing is hashed; the
//                   report's root and counts are zero.
//     ORDER         numbers[seq] <= numbers[seq - 1]; witness = the lowest such
//                   seq >= 1
//     CREDIT_RULE   an entry's credited bit != "no earlier entry has this
//                   nullifier"; witness = the lowest such seq, first = the
//                   lowest seq holding that nullifier
//     TOTALS        claimed (credited, limb sums) != those of the entries whose
//                   credited bit is set
//     PAYOUTS       the claimed list != the log's payouts (per account the limb
//                   sums of its entries with the credited bit, the accounts in
//                   the order of their first such entry); witness = the lowest
//                   i < min(A, K) where account, sums or first_seq differ, else,
//                   A != K, min(A, K)
//     ROOT          a claimed root != the log tree's root over [0, n)
//     COMMITMENT    some (root_i, n_i) has n_i > n, or the root of the prefix
//                   [0, n_i) != root_i; witness = the lowest such index i
//   On every status but NON_CANONICAL the report carries the recomputed root,
//   credited, the four limb sums and the account count.  Limb sums are compared
//   as the totals they name (ledger_table.h's sums_equal), so a claim may split
//   an exact total into limbs in any way.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "audit_common.h"
#include "ledger_log.h"

namespace ql {

// qp_ledger_audit_status (qpgpu.h)
enum : uint32_t { AUDIT_OK = 0, AUDIT_NON_CANONICAL = 1, AUDIT_ORDER = 2, AUDIT_CREDIT_RULE = 3, AUDIT_TOTALS = 4,
                  AUDIT_PAYOUTS = 5, AUDIT_ROOT = 6, AUDIT_COMMITMENT = 7 };
using qpk::AUDIT_NONE;

// the nouns of a ledger's texts, stated once: qp_ledger (ledger.cpp) inherits them for handle_common.h's
struct Words {
  static constexpr const char *HANDLE = "ledger", *ENTRY = "transfer", *ABI = "qp_ledger";
};

// qp_ledger_audit_report
struct AuditReport {
  uint32_t status, pad;
  uint64_t witness, first;
  uint64_t root[4], credited, sums[4], accounts;
};

// a published log
struct AuditLog {
  const uint64_t *nullifiers = nullptr, *numbers = nullptr;  // [n][4], [n]
  const uint32_t *amounts = nullptr;                         // [n][4]
  const uint64_t *accounts = nullptr;                        // [n][4]
  const uint8_t *flags = nullptr;                            // [n]
  uint64_t n = 0;
};

// the claims published beside a log; a null pointer: not claimed
struct AuditClaims {
  const uint64_t *root = nullptr;           // [4]
  const uint64_t *totals = nullptr;         // [5]: credited, the four limb sums
  const uint64_t *pay_accounts = nullptr;   // [npay][4]; null: the payouts are not claimed
  const uint64_t *pay_sums = nullptr;       // [npay][4]
  const uint64_t *pay_first_seq = nullptr;  // [npay]
  uint64_t npay = 0;
  const uint64_t *commit_roots = nullptr;  // [ncommit][4]
  const uint64_t *commit_ns = nullptr;     // [ncommit]
  uint32_t ncommit = 0;
};

// what the passes over a log found, on either path: the lowest offender of each of the first three
// reasons (AUDIT_NONE: none), the owner of the credit rule's, the counts, the lowest claimed payout
// below min(accounts, npay) that differs, the root
struct AuditFacts {
  uint64_t non_canonical = AUDIT_NONE, order = AUDIT_NONE, credit_rule = AUDIT_NONE, first = AUDIT_NONE;
  uint64_t credited = 0, sums[4] = {0, 0, 0, 0}, accounts = 0;
  uint64_t payout = AUDIT_NONE;
  uint64_t root[4] = {0, 0, 0, 0};
};

inline bool entry_canonical(const AuditLog &g, uint64_t seq) {
  return canonical(g.nullifiers + seq * 4, 4) && canonical(g.accounts + seq * 4, 4) && g.numbers[seq] < P &&
         g.flags[seq] <= FLAG_CREDITED;
}

// the report of a log whose first pass found a non-canonical entry: nothing was hashed
inline void audit_non_canonical(uint64_t witness, AuditReport &r) {
  r = AuditReport{AUDIT_NON_CANONICAL, 0, witness, AUDIT_NONE, {0, 0, 0, 0}, 0, {0, 0, 0, 0}, 0};
}

// The verdict from the facts of a canonical log of n entries, the same on both paths: the first
// reason in the table's order.  prefix_root(i, m, out[4]), 1 <= m <= n, is asked only when no earlier
// reason fired.
template <class PrefixRoot>
inline void audit_verdict(const AuditFacts &f, uint64_t n, const AuditClaims &c, PrefixRoot prefix_root, AuditReport &r) {
  r = AuditReport{AUDIT_OK, 0, AUDIT_NONE, AUDIT_NONE, {f.root[0], f.root[1], f.root[2], f.root[3]}, f.credited,
                  {f.sums[0], f.sums[1], f.sums[2], f.sums[3]}, f.accounts};
  if (f.order != AUDIT_NONE) {
    r.status = AUDIT_ORDER;
    r.witness = f.order;
  } else if (f.credit_rule != AUDIT_NONE) {
    r.status = AUDIT_CREDIT_RULE;
    r.witness = f.credit_rule;
    r.first = f.first;
  } else if (c.totals && (c.totals[0] != f.credited || !sums_equal(c.totals + 1, f.sums))) {
    r.status = AUDIT_TOTALS;
  } else if (c.pay_accounts && (f.payout != AUDIT_NONE || c.npay != f.accounts)) {
    r.status = AUDIT_PAYOUTS;
    r.witness = f.payout != AUDIT_NONE ? f.payout : (c.npay < f.accounts ? c.npay : f.accounts);
  } else if (c.root && memcmp(c.root, f.root, 32)) {
    r.status = AUDIT_ROOT;
  } else {
    const uint64_t i = qpk::broken_commitment(c.commit_roots, c.commit_ns, c.ncommit, n, prefix_root);
    if (i != AUDIT_NONE) {
      r.status = AUDIT_COMMITMENT;
      r.witness = i;
    }
  }
}

// what the ABI call refuses before any audit runs: "" when the arguments are usable
inline std::string audit_refusal(const AuditLog &g, const AuditClaims &c) {
  if (!g.nullifiers || !g.numbers || !g.amounts || !g.accounts || !g.flags) return "null buffer";
  if (!g.n || g.n > MAX_CAPACITY) return "a log of " + std::to_string(g.n) + " entries: an audit takes 1 to 2^31";
  if (c.root && !canonical(c.root, 4)) return "the claimed root is not four canonical field elements";
  if (c.pay_accounts && c.npay && (!c.pay_sums || !c.pay_first_seq)) return "null payouts buffer";
  if (c.pay_accounts)
    for (uint64_t i = 0; i < c.npay; i++)
      if (!canonical(c.pay_accounts + i * 4, 4))
        return "the account of claimed payout " + std::to_string(i) + " is not four canonical field elements";
  return qpk::commitment_refusal(c.commit_roots, c.commit_ns, c.ncommit);
}

// the first pass of the host path: the lowest non-canonical entry, the lowest entry out of order
inline void audit_screen_host(const AuditLog &g, AuditFacts &f) {
  for (uint64_t seq = 0; seq < g.n && f.non_canonical == AUDIT_NONE; seq++)
    if (!entry_canonical(g, seq)) f.non_canonical = seq;
  for (uint64_t seq = 1; seq < g.n && f.order == AUDIT_NONE; seq++)
    if (g.numbers[seq] <= g.numbers[seq - 1]) f.order = seq;
}

// The host path, sequentially.  The log goes into `led` (opened here for n): every entry probes the
// nullifier table in seq order, so a slot's owner is the lowest seq of its nullifier; the flags are
// read and never written, and an entry whose flag says credited is credited.  Afterwards `led` holds
// both tables, the sums and the payees of that log, and `log` the log tree over [0, n).  false: the
// log is not canonical (f.non_canonical is set, nothing else was done).  A restore opens `led` for the
// new ledger's capacity >= n, and then `led` is the ledger of that log; it leaves the tree out
// (want_root false: `log` is not touched and f.root stays zero) and commits the ledger it got.
inline bool audit_facts_host(const AuditLog &g, const AuditClaims &c, HostLedger &led, HostLog &log, AuditFacts &f,
                             uint64_t capacity = 0, bool want_root = true) {
  f = AuditFacts();
  audit_screen_host(g, f);
  if (f.non_canonical != AUDIT_NONE) return false;
  const uint64_t n = g.n;
  led = HostLedger();
  led.open(capacity ? capacity : n);
  led.nullifier.assign(g.nullifiers, g.nullifiers + n * 4);
  led.number.assign(g.numbers, g.numbers + n);
  led.amount.assign(g.amounts, g.amounts + n * 4);
  led.account.assign(g.accounts, g.accounts + n * 4);
  led.flags.assign(g.flags, g.flags + n);
  led.astay.assign(n, EMPTY);
  for (uint64_t seq = 0; seq < n; seq++) {
    const uint32_t owner = led.nslot[led.ntable().probe((uint32_t)seq)];
    const bool credited = g.flags[seq] & FLAG_CREDITED;
    if (credited != (owner == seq) && f.credit_rule == AUDIT_NONE) {
      f.credit_rule = seq;
      f.first = owner;
    }
    if (!credited) continue;
    led.credited++;
    led.credit((uint32_t)seq);
    if (led.aslot[led.astay[seq]] == seq) led.payee.push_back((uint32_t)seq);
    for (int j = 0; j < 4; j++) f.sums[j] += g.amounts[seq * 4 + j];
  }
  f.credited = led.credited;
  f.accounts = led.accounts();
  if (c.pay_accounts) {
    const uint64_t k = c.npay < f.accounts ? c.npay : f.accounts;
    for (uint64_t i = 0; i < k && f.payout == AUDIT_NONE; i++) {
      const uint32_t seq = led.payee[i];
      if (!key_equal(c.pay_accounts + i * 4, &led.account[(size_t)seq * 4]) ||
          !sums_equal(c.pay_sums + i * 4, &led.sum[(size_t)led.astay[seq] * 4]) || c.pay_first_seq[i] != seq)
        f.payout = i;
    }
  }
  if (!want_root) return true;
  log.open(n);
  log.leaves(g.nullifiers, g.numbers, g.amounts, g.accounts, g.flags, 0, n);
  log.append(n, log_node);
  memcpy(f.root, log.root(), 32);
  return true;
}

// qp_ledger_log_audit without a context; the caller ran audit_refusal
inline void audit_host(const AuditLog &g, const AuditClaims &c, AuditReport &r) {
  HostLedger led;
  HostLog log;
  AuditFacts f;
  if (!audit_facts_host(g, c, led, log, f)) return audit_non_canonical(f.non_canonical, r);
  audit_verdict(f, g.n, c, [&log](uint32_t, uint64_t m, uint64_t out[4]) { log.prefix_root(m, log_node, out); }, r);
}

// ---- qp_ledger_restore: a ledger reopened from a published log.  It runs the audit's reasons 1-3 on
// the new ledger's own buffers, and 6 (the root) when one is expected; the claims of reasons 4, 5 and 7
// are not part of a restore.

// what a restore refuses beside a failing audit: "" when (capacity, cast_count) fit the log
inline std::string restore_refusal(const uint64_t *numbers, uint64_t n, uint64_t capacity, uint64_t cast_count) {
  return qpk::restore_refusal(numbers, n, capacity, cast_count, Words::HANDLE, Words::ENTRY);
}

// the verdict of a restore from the facts of a canonical log; root: the expected root, with f.root the
// restored ledger's commitment, or null
inline void restore_verdict(const AuditFacts &f, uint64_t n, const uint64_t *root, AuditReport &r) {
  AuditClaims c;
  c.root = root;
  audit_verdict(f, n, c, [](uint32_t, uint64_t, uint64_t *) {}, r);
}

// the words qp_wormhole.LEDGER_AUDIT_STATUS_TEXT has for a status
inline const char *audit_status_text(uint32_t status) {
  static const char *const text[] = {"ok", "non-canonical entry", "transfer numbers out of order", "credit rule broken",
                                     "claimed totals differ", "claimed payouts differ", "claimed root differs",
                                     "earlier commitment does not hold"};
  return status <= AUDIT_COMMITMENT ? text[status] : "unknown status";
}

// the reason and the witness of a failing audit, for a refusal's message
inline std::string audit_failure_text(const AuditReport &r) {
  return qpk::audit_failure_text(audit_status_text(r.status), r.witness, r.first, r.status == AUDIT_COMMITMENT);
}

}  // namespace ql
