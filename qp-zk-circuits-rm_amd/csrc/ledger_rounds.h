// ledger_rounds.h — payout rounds in host C++: what a range [m0, m1) of the
// transfer log pays, the refusals of the two entry points and the host path.
// Plain C++ next to ledger_table.h (no HIP beyond QL_HD); included by
// ledger.cpp, ledger_rounds.cpp, ledger.hip (the device credit kernel asks
// round_credits, so both paths run one statement of the rule) and the
// stand-alone check tools/ledger_restore_check.cpp.
//
// Definitions (DESIGN §14 and qpgpu.h state the same):
//   A settler pays per round: per published commitment (root_k, n_k).  Round k
//   pays the log entries [n_{k-1}, n_k).  The payouts of a range [m0, m1), 0 <=
//   m0 <= m1 <= n, are one row per account that has an entry seq with m0 <= seq
//   < m1 and flags bit 0 (credited) set:
//     account, the four limb sums over those entries, first_seq = the lowest
//     such seq
//   in first_seq order.  Entries outside the range do not count: an account
//   credited before m0 and again inside appears with its in-range sums and its
//   in-range first_seq.  The flags are trusted, as the payouts and the recount
//   trust them; the audit is what checks flags.  [0, n) gives the cumulative
//   payouts; the rounds of consecutive ranges add up to them account by account.
//   m0 == m1 gives no rows.
// Both paths use a scratch account table of the call's own, a slot table
// (slot_table.h) of table_slots(m1 - m0) slots keyed by the account.  The
// ledger and the log are only read.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "ledger_table.h"

namespace ql {

// the rule: an entry inside the range counts iff its credited bit is set
QL_HD inline bool round_credits(uint8_t flags) { return flags & FLAG_CREDITED; }

// the rows of one range: accounts [rows][4], sums [rows][4], first_seq [rows]
struct RoundRows {
  std::vector<uint64_t> accounts, sums, first_seq;
  uint64_t count() const { return first_seq.size(); }
};

// what both entry points refuse before anything runs: "" when the range lies in a log of n entries
// and the output buffers fit cap
inline std::string round_refusal(uint64_t n, uint64_t m0, uint64_t m1, uint64_t cap, const uint64_t *accounts,
                                 const uint64_t *sums, const uint64_t *first_seq, const uint64_t *count) {
  if (!count) return "null count";
  if (m0 > m1 || m1 > n)
    return "entries [" + std::to_string(m0) + ", " + std::to_string(m1) + ") are not a range of the log's " +
           std::to_string(n);
  if (cap && (!accounts || !sums || !first_seq)) return "null buffer for " + std::to_string(cap) + " rows";
  return "";
}

// the log-only form reads a log nobody screened: the entries of the range must be a ledger's (the
// entries outside it are not read)
inline std::string round_log_refusal(const uint64_t *accounts_log, const uint8_t *flags, uint64_t m0, uint64_t m1) {
  for (uint64_t seq = m0; seq < m1; seq++) {
    if (!canonical(accounts_log + seq * 4, 4))
      return "the account of entry " + std::to_string(seq) + " is not four canonical field elements";
    if (flags[seq] > FLAG_CREDITED) return "the flags of entry " + std::to_string(seq) + " are above 1";
  }
  return "";
}

// The host path, sequentially, over a log in the layout qp_ledger_entries gives (indexed by seq from
// 0).  Entries arrive in seq order, so an account's row is made by its first credited entry of the
// range and the rows come out in first_seq order.  A slot holds a row's index, and a row exists only
// once its slot is claimed, so the probing key is not in the table's key column yet: the probe is
// written out here and not qst::SlotTable's, which takes the key from keys[seq].
inline void round_payouts_host(const uint64_t *accounts_log, const uint32_t *amounts, const uint8_t *flags, uint64_t m0,
                               uint64_t m1, RoundRows &out) {
  out = RoundRows();
  if (m0 == m1) return;
  const uint64_t mask = table_slots(m1 - m0) - 1;
  std::vector<uint32_t> slot(mask + 1, EMPTY);
  for (uint64_t seq = m0; seq < m1; seq++) {
    if (!round_credits(flags[seq])) continue;
    const uint64_t *key = accounts_log + seq * 4;
    uint64_t at = key[0] & mask;
    for (;; at = (at + 1) & mask) {  // rows <= m1 - m0 <= S / 2: an empty slot exists
      if (slot[at] == EMPTY) {
        slot[at] = (uint32_t)out.count();
        out.accounts.insert(out.accounts.end(), key, key + 4);
        out.sums.insert(out.sums.end(), 4, 0);
        out.first_seq.push_back(seq);
        break;
      }
      if (key_equal(&out.accounts[(size_t)slot[at] * 4], key)) break;
    }
    for (int j = 0; j < 4; j++) out.sums[(size_t)slot[at] * 4 + j] += amounts[seq * 4 + j];
  }
}

// the first min(cap, rows) rows into the caller's arrays, *count = rows
inline void round_store(const RoundRows &rows, uint64_t cap, uint64_t *accounts, uint64_t *sums, uint64_t *first_seq,
                        uint64_t *count) {
  const uint64_t k = rows.count() < cap ? rows.count() : cap;
  if (k) {
    memcpy(accounts, rows.accounts.data(), k * 32);
    memcpy(sums, rows.sums.data(), k * 32);
    memcpy(first_seq, rows.first_seq.data(), k * 8);
  }
  *count = rows.count();
}

}  // namespace ql
