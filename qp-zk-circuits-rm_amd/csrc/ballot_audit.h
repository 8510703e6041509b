// ballot_audit.h — the audit of a published ballot log in host C++: the seven
// reasons and their witnesses, the verdict both paths share, and the host path
// itself (HostBox's probe gives the owner, HostLog the root and the prefix
// roots).  The commitment claims, a restore's refusals and the text of a failing
// audit are audit_common.h's, shared with the transfer log.  Plain C++ next to
// ballot_log.h (no HIP).  Included by ballot.cpp, ballot_audit.cpp and the
// stand-alone check tools/ballot_audit_check.cpp.
//
// Definitions (DESIGN §13 and qpgpu.h state the same):
//   A published log is what qp_ballot_box_entries returns: nullifiers[n][4],
//   numbers[n], flags[n], 1 <= n <= 2^31.  Beside it come optional claims: a
//   root, a tally (yes, no), earlier commitments (root_i, n_i).  The audit
//   reports the first reason that fires, in this order, and the lowest
//   offender as its witness, so the report is a function of the input alone:
//     OK            nothing below
//     NON_CANONICAL a nullifier felt >= p, a number >= p or a flags byte > 3;
//                   witness = the lowest such seq.  Nothing is hashed; the
//                   report's root and counts are zero.
//     ORDER         numbers[seq] <= numbers[seq - 1] (a box's log has strictly
//                   increasing numbers); witness = the lowest such seq >= 1
//     COUNT_RULE    an entry's counted bit != "no earlier entry has this
//                   nullifier"; witness = the lowest such seq, first = the
//                   lowest seq holding that nullifier
//     TALLY         a tally is claimed and differs from (counted & vote,
//                   counted & !vote) of the flags
//     ROOT          a root is claimed and differs from the log tree's root over [0, n)
//     COMMITMENT    some (root_i, n_i) has n_i > n, or the root of the prefix
//                   [0, n_i) != root_i; witness = the lowest such index i
//   On every status but NON_CANONICAL the report carries the recomputed root
//   and (yes, no, counted) of the flags.
//   Prefix root of m, 1 <= m <= n, in a tree of n leaves (acc_layout.h's
//   HostTree::prefix_root): acc = leaf m - 1; at each level l while
//   c = ceil(m / 2^l) > 1: c odd, acc moves up unchanged; c even,
//   acc = H(dig[l][c - 2] || acc).  dig[l][c - 2] covers only leaves below m,
//   so it is the same digest in the larger tree; the prefix root at m = n is
//   the root.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "audit_common.h"
#include "ballot_log.h"

namespace qb {

// qp_audit_status (qpgpu.h)
enum : uint32_t { AUDIT_OK = 0, AUDIT_NON_CANONICAL = 1, AUDIT_ORDER = 2, AUDIT_COUNT_RULE = 3, AUDIT_TALLY = 4,
                  AUDIT_ROOT = 5, AUDIT_COMMITMENT = 6 };
using qpk::AUDIT_NONE;

// the nouns of a box's texts, stated once: qp_ballot_box (ballot.cpp) inherits them for handle_common.h's
struct Words {
  static constexpr const char *HANDLE = "box", *ENTRY = "ballot", *ABI = "qp_ballot_box";
};

// qp_audit_report
struct AuditReport {
  uint32_t status, pad;
  uint64_t witness, first;
  uint64_t root[4], yes, no, counted;
};

// the claims published beside a log; a null pointer: not claimed
struct AuditClaims {
  const uint64_t *root = nullptr;          // [4]
  const uint64_t *tally = nullptr;         // [2]: yes, no
  const uint64_t *commit_roots = nullptr;  // [ncommit][4]
  const uint64_t *commit_ns = nullptr;     // [ncommit]
  uint32_t ncommit = 0;
};

// what the passes over a log found, on either path: the lowest offender of each of the first three
// reasons (AUDIT_NONE: none), the owner of the count rule's, the counts of the flags, the root
struct AuditFacts {
  uint64_t non_canonical = AUDIT_NONE, order = AUDIT_NONE, count_rule = AUDIT_NONE, first = AUDIT_NONE;
  uint64_t yes = 0, no = 0, counted = 0;
  uint64_t root[4] = {0, 0, 0, 0};
};

inline const char *audit_status_text(uint32_t status) {
  static const char *const text[] = {"ok", "a non-canonical entry", "ballot numbers out of order",
                                     "the count rule is broken", "the claimed tally differs",
                                     "the claimed root differs", "an earlier commitment does not hold"};
  return status < 7 ? text[status] : "?";
}

inline bool entry_canonical(const uint64_t nul[4], uint64_t number, uint8_t flags) {
  return canonical(nul, 4) && number < P && flags <= (FLAG_VOTE | FLAG_COUNTED);
}

// the report of a log whose first pass found a non-canonical entry: nothing was hashed
inline void audit_non_canonical(uint64_t witness, AuditReport &r) {
  r = AuditReport{AUDIT_NON_CANONICAL, 0, witness, AUDIT_NONE, {0, 0, 0, 0}, 0, 0, 0};
}

// The verdict from the facts of a canonical log of n entries, the same on both
// paths: the first reason in the table's order.  prefix_root(m, out[4]), 1 <= m
// <= n, is asked only when no earlier reason fired.  `reasons`: a bit per
// status that may be reported (restore leaves the tally and the commitments out).
template <class PrefixRoot>
inline void audit_verdict(const AuditFacts &f, uint64_t n, const AuditClaims &c, uint32_t reasons, PrefixRoot prefix_root,
                          AuditReport &r) {
  r = AuditReport{AUDIT_OK, 0, AUDIT_NONE, AUDIT_NONE, {f.root[0], f.root[1], f.root[2], f.root[3]}, f.yes, f.no, f.counted};
  auto on = [reasons](uint32_t s) { return reasons >> s & 1; };
  if (on(AUDIT_ORDER) && f.order != AUDIT_NONE) {
    r.status = AUDIT_ORDER;
    r.witness = f.order;
  } else if (on(AUDIT_COUNT_RULE) && f.count_rule != AUDIT_NONE) {
    r.status = AUDIT_COUNT_RULE;
    r.witness = f.count_rule;
    r.first = f.first;
  } else if (on(AUDIT_TALLY) && c.tally && (c.tally[0] != f.yes || c.tally[1] != f.no)) {
    r.status = AUDIT_TALLY;
  } else if (on(AUDIT_ROOT) && c.root && memcmp(c.root, f.root, 32)) {
    r.status = AUDIT_ROOT;
  } else if (on(AUDIT_COMMITMENT)) {
    const uint64_t i = qpk::broken_commitment(c.commit_roots, c.commit_ns, c.ncommit, n, prefix_root);
    if (i != AUDIT_NONE) {
      r.status = AUDIT_COMMITMENT;
      r.witness = i;
    }
  }
}
constexpr uint32_t AUDIT_ALL_REASONS = 0x7E, AUDIT_RESTORE_REASONS = 1u << AUDIT_ORDER | 1u << AUDIT_COUNT_RULE | 1u << AUDIT_ROOT;

// what an ABI call refuses before any audit runs: "" when the arguments are
// usable (n_i == 0 and a non-canonical claimed root are QP_ERR_ARG, not audit results)
inline std::string audit_refusal(uint64_t n, const AuditClaims &c) {
  if (!n || n > MAX_CAPACITY) return "a log of " + std::to_string(n) + " entries: an audit takes 1 to 2^31";
  if (c.root && !canonical(c.root, 4)) return "the claimed root is not four canonical field elements";
  return qpk::commitment_refusal(c.commit_roots, c.commit_ns, c.ncommit);
}

// the first pass of the host path: the lowest non-canonical entry, the lowest entry out of order
inline void audit_screen_host(const uint64_t *nullifiers, const uint64_t *numbers, const uint8_t *flags, uint64_t n,
                              AuditFacts &f) {
  for (uint64_t seq = 0; seq < n && f.non_canonical == AUDIT_NONE; seq++)
    if (!entry_canonical(nullifiers + seq * 4, numbers[seq], flags[seq])) f.non_canonical = seq;
  for (uint64_t seq = 1; seq < n && f.order == AUDIT_NONE; seq++)
    if (numbers[seq] <= numbers[seq - 1]) f.order = seq;
}

// The host path, sequentially.  The log goes into `box` (opened here for
// `capacity` >= n): every entry probes in seq order, so a slot's owner is the
// lowest seq of its nullifier; the flags are read and never written.  Afterwards
// `box` is the box of that log (table, tally from the flags).  With want_root the
// log tree over [0, n) is built in `log` (laid out for n).  false: the log is
// not canonical (f.non_canonical is set, nothing else was done).
inline bool audit_facts_host(const uint64_t *nullifiers, const uint64_t *numbers, const uint8_t *flags, uint64_t n,
                             uint64_t capacity, bool want_root, HostBox &box, HostLog &log, AuditFacts &f) {
  f = AuditFacts();
  audit_screen_host(nullifiers, numbers, flags, n, f);
  if (f.non_canonical != AUDIT_NONE) return false;
  box = HostBox();
  box.open(capacity);
  box.nullifier.assign(nullifiers, nullifiers + n * 4);
  box.number.assign(numbers, numbers + n);
  box.flags.assign(flags, flags + n);
  for (uint64_t seq = 0; seq < n; seq++) {
    const uint32_t owner = box.slot[box.table().probe((uint32_t)seq)];
    const bool counted = flags[seq] & FLAG_COUNTED;
    if (counted != (owner == seq) && f.count_rule == AUDIT_NONE) {
      f.count_rule = seq;
      f.first = owner;
    }
    if (counted) {
      f.counted++;
      (flags[seq] & FLAG_VOTE ? f.yes : f.no)++;
    }
  }
  box.yes = f.yes;
  box.no = f.no;
  if (want_root) {
    log.open(n);
    for (uint64_t seq = 0; seq < n; seq++) log_leaf(nullifiers + seq * 4, numbers[seq], flags[seq], log.node(0, seq));
    log.append(n, log_node);
    memcpy(f.root, log.root(), 32);
  }
  return true;
}

// qp_ballot_log_audit without a context; the caller ran audit_refusal
inline void audit_host(const uint64_t *nullifiers, const uint64_t *numbers, const uint8_t *flags, uint64_t n,
                       const AuditClaims &c, uint32_t reasons, AuditReport &r) {
  HostBox box;
  HostLog log;
  AuditFacts f;
  if (!audit_facts_host(nullifiers, numbers, flags, n, n, true, box, log, f)) return audit_non_canonical(f.non_canonical, r);
  audit_verdict(f, n, c, reasons, [&log](uint32_t, uint64_t m, uint64_t out[4]) { log.prefix_root(m, log_node, out); }, r);
}

// what a restore refuses beside a failing audit: "" when (capacity, cast_count) fit the log
inline std::string restore_refusal(const uint64_t *numbers, uint64_t n, uint64_t capacity, uint64_t cast_count) {
  return qpk::restore_refusal(numbers, n, capacity, cast_count, Words::HANDLE, Words::ENTRY);
}

// the reason and the witness of a failing audit, for a refusal's message
inline std::string audit_failure_text(const AuditReport &r) {
  return qpk::audit_failure_text(audit_status_text(r.status), r.witness, r.first, r.status == AUDIT_COMMITMENT);
}

}  // namespace qb
