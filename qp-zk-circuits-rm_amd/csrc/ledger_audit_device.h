// ledger_audit_device.h — what ledger_audit.cpp (qp_ledger_log_audit) shares
// with ledger.cpp beside the headers of the kernels and of the rules: the device
// half of a ledger for one capacity (the ledger holds one, a reserve builds the
// next beside it, an audit one for its call) and the passes over an uploaded log
// that the audit and qp_ledger_restore both run.
#pragma once
#include <string>
#include "acc_tree.h"
#include "ctx.h"
#include "ledger_audit.h"
#include "ledger_kernels.h"
#include "ledger_table.h"

namespace qla {

// the device half of a ledger for one capacity: the log, the two tables, the sums
struct LedgerTables {
  DevBuf nul, num, amt, acc, flags, astay, nslot, aslot, sum;
  uint64_t mask = 0;
  qpk::LedgerDev dev() const {
    return qpk::LedgerDev{nul.p,          num.p,
                          amt.as<uint32_t>(),   acc.p,
                          flags.as<uint8_t>(),  astay.as<uint32_t>(),
                          nslot.as<uint32_t>(), aslot.as<uint32_t>(),
                          sum.as<unsigned long long>(), mask};
  }
};

// t for `capacity` entries, both tables all-empty and the sums zero (memsets enqueued on s)
inline int alloc_tables(AccErr e, hipStream_t s, uint64_t capacity, LedgerTables &t) {
  const uint64_t S = ql::table_slots(capacity);
  QP_HIP_TRY(&e, t.nul.alloc(capacity * 4));
  QP_HIP_TRY(&e, t.num.alloc(capacity));
  QP_HIP_TRY(&e, t.amt.alloc(capacity * 2));
  QP_HIP_TRY(&e, t.acc.alloc(capacity * 4));
  QP_HIP_TRY(&e, t.flags.alloc((capacity + 7) / 8));
  QP_HIP_TRY(&e, t.astay.alloc((capacity + 1) / 2));
  QP_HIP_TRY(&e, t.nslot.alloc(S / 2));
  QP_HIP_TRY(&e, t.aslot.alloc(S / 2));
  QP_HIP_TRY(&e, t.sum.alloc(S * 4));
  t.mask = S - 1;
  QP_HIP_TRY(&e, hipMemsetAsync(t.nslot.p, 0xFF, S * 4, s));
  QP_HIP_TRY(&e, hipMemsetAsync(t.aslot.p, 0xFF, S * 4, s));
  QP_HIP_TRY(&e, hipMemsetAsync(t.sum.p, 0, S * 32, s));
  return QP_OK;
}

// the scratch of the passes below, kept by their caller until its last synchronise: the device
// report, the insert's stay words, and the report's host copy as of the last download
struct AuditPasses {
  DevBuf d_rep, d_stay;
  qpk::LedgerAuditDev h;
  qpk::LedgerAuditDev *rep() const { return d_rep.as<qpk::LedgerAuditDev>(); }
  // the lowest entry out of order and the lowest that breaks the credit rule, from h into f
  void rule_facts(ql::AuditFacts &f) const {
    if (h.order != qpk::LEDGER_AUDIT_NO_SEQ) f.order = h.order;
    if (h.credit_rule != ~0ull) {
      f.credit_rule = h.credit_rule >> 32;
      f.first = h.credit_rule & 0xFFFFFFFFu;
    }
  }
};

// The passes over log g that the audit and the restore share, on d (sized for >= g.n entries, both
// tables all-empty, the sums zero; the caller has set the device): one upload of the log; the
// audit's screen; a synchronise, where a non-canonical log ends (*canonical false, a.h.non_canonical
// its witness, nothing inserted or hashed); the whole-log insert into the nullifier table; the audit's
// resolve, a launch of its own, which reads the final slot words for the credit rule and credits the
// flagged entries into the account table and the sums.  Returns with the resolve launched and not
// waited for: the caller enqueues what it adds, downloads the report into a.h and synchronises.
int audit_screen_insert_resolve(AccErr e, hipStream_t s, const ql::AuditLog &g, const qpk::LedgerDev &d, AuditPasses &a,
                                bool *canonical);

// the reason of a call that has no ledger to carry it: qp_ledger_last_error(NULL)'s text on this
// thread, and c's err when there is a context (ledger.cpp)
void set_ledgerless_error(qp_ctx *c, const std::string &why);

// The scratch of a payout round and what its credit leaves there: the view's account table (aslot,
// sum), astay [k], the owners of the range compacted in log order (payee [rows], local indices j =
// seq - m0) and their number.
struct RoundCredit {
  DevBuf astay, aslot, sum, d_err, d_blk, d_payee;
  qpk::LedgerDev v{};  // the view (ledger_kernels.h): account, amount and flags at entry m0, the scratch tables
  uint32_t rows = 0;
  const uint32_t *payee() const { return d_payee.as<uint32_t>(); }
};

// The credit of a range into r and the owners' compaction (ledger_rounds.cpp): the scratch's
// allocation and memsets, ledger_round_credit, ledger_payee_count, ledger_scan, ledger_payee_write,
// and one synchronise that reads r.rows and the defensive error word.  The first half of
// rounds_device, and of a claims commitment's device build (claims_commit.h): one statement for both.
int round_credit_device(qp_ctx *c, std::string &err, const uint64_t *accounts_at_m0, const uint32_t *amounts_at_m0,
                        const uint8_t *flags_at_m0, uint64_t k, RoundCredit &r);

// The device path of a payout round (ledger_rounds.cpp), shared by qp_ledger_payouts_between (the
// pointers lead into the ledger's own log, which is only read) and qp_ledger_log_payouts_between (into
// the uploaded range): accounts, amounts and flags are device pointers at entry m0, k = m1 - m0 >= 1.
// The first min(cap, rows) rows into the host arrays, first_seq as log indices; *count = rows.  A
// failure leaves its reason in err.
int rounds_device(qp_ctx *c, std::string &err, const uint64_t *accounts_at_m0, const uint32_t *amounts_at_m0,
                  const uint8_t *flags_at_m0, uint64_t k, uint64_t m0, uint64_t cap, uint64_t *accounts, uint64_t *sums,
                  uint64_t *first_seq, uint64_t *count);

}  // namespace qla
