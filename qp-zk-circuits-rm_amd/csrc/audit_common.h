// audit_common.h — what the audit of a ballot log (ballot_audit.h) and of a
// transfer log (ledger_audit.h) state in the same words: the commitment claims
// (root_i, n_i), a restore's refusals and the text of a failing audit.  Each
// of qb:: and ql:: keeps its own statuses, report, facts, claims and the
// reasons that are its own.  Plain C++ (no HIP).
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include "slot_table.h"

namespace qpk {

constexpr uint64_t AUDIT_NONE = ~0ull;  // no witness, no first

// The commitment reason of a verdict over a log of n entries: the lowest i whose (root_i, n_i) has
// n_i > n or whose root differs from the root of the prefix [0, n_i); AUDIT_NONE when all hold.
// prefix_root(i, m, out[4]), 1 <= m <= n, is asked for the claims that name a prefix, in order.
template <class PrefixRoot>
inline uint64_t broken_commitment(const uint64_t *commit_roots, const uint64_t *commit_ns, uint32_t ncommit, uint64_t n,
                                  PrefixRoot &prefix_root) {
  for (uint32_t i = 0; i < ncommit; i++) {
    uint64_t got[4];
    if (commit_ns[i] > n) return i;
    prefix_root(i, commit_ns[i], got);
    if (memcmp(got, commit_roots + (size_t)i * 4, 32)) return i;
  }
  return AUDIT_NONE;
}

// what an audit's ABI call refuses in the commitment claims before any audit runs: "" when they are
// usable (n_i == 0 and a non-canonical root are QP_ERR_ARG, not audit results)
inline std::string commitment_refusal(const uint64_t *commit_roots, const uint64_t *commit_ns, uint32_t ncommit) {
  if (ncommit && (!commit_roots || !commit_ns)) return "null commitment buffer";
  for (uint32_t i = 0; i < ncommit; i++) {
    if (!commit_ns[i]) return "commitment " + std::to_string(i) + " names n = 0";
    if (!qst::canonical(commit_roots + (size_t)i * 4, 4))
      return "the root of commitment " + std::to_string(i) + " is not four canonical field elements";
  }
  return "";
}

// what a restore refuses beside a failing audit: "" when (capacity, cast_count) fit the log.
// handle / entry: the two nouns ("box", "ballot").
inline std::string restore_refusal(const uint64_t *numbers, uint64_t n, uint64_t capacity, uint64_t cast_count,
                                   const char *handle, const char *entry) {
  if (n > qst::MAX_CAPACITY) return "a log of " + std::to_string(n) + " entries: a " + handle + " holds at most 2^31";
  if (!capacity || capacity > qst::MAX_CAPACITY || capacity < n)
    return "capacity " + std::to_string(capacity) + " for a log of " + std::to_string(n) +
           " entries: it must hold them (and at least one) and be at most 2^31";
  if (n && cast_count <= numbers[n - 1])
    return "cast_count " + std::to_string(cast_count) + " is not above the log's last " + entry + " number " +
           std::to_string(numbers[n - 1]);
  return "";
}

// The reason and the witness of a failing audit, for a refusal's message.  commitment: the witness
// is the index of a commitment claim, not a log entry.  A restore claims no commitments, so today
// only qp_ballot_box_restore and qp_ledger_restore reach this and never with a commitment witness.
inline std::string audit_failure_text(const char *status_text, uint64_t witness, uint64_t first, bool commitment) {
  std::string s = std::string("the log fails its audit: ") + status_text;
  if (witness != AUDIT_NONE) s += (commitment ? " (commitment " : " (entry ") + std::to_string(witness);
  if (first != AUDIT_NONE) s += ", its nullifier first at entry " + std::to_string(first);
  if (witness != AUDIT_NONE) s += ")";
  return s;
}

}  // namespace qpk
