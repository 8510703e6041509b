// ledger_audit_device.h — what ledger_audit.cpp (qp_ledger_log_audit) shares
// with ledger.cpp beside the headers of the kernels and of the rules.
#pragma once
#include <string>
#include "ctx.h"

namespace qla {

// the reason of a call that has no ledger to carry it: qp_ledger_last_error(NULL)'s text on this
// thread, and c's err when there is a context (ledger.cpp)
void set_ledgerless_error(qp_ctx *c, const std::string &why);

// The device path of a payout round (ledger_rounds.cpp), shared by qp_ledger_payouts_between (the
// pointers lead into the ledger's own log, which is only read) and qp_ledger_log_payouts_between (into
// the uploaded range): accounts, amounts and flags are device pointers at entry m0, k = m1 - m0 >= 1.
// The first min(cap, rows) rows into the host arrays, first_seq as log indices; *count = rows.  A
// failure leaves its reason in err.
int rounds_device(qp_ctx *c, std::string &err, const uint64_t *accounts_at_m0, const uint32_t *amounts_at_m0,
                  const uint8_t *flags_at_m0, uint64_t k, uint64_t m0, uint64_t cap, uint64_t *accounts, uint64_t *sums,
                  uint64_t *first_seq, uint64_t *count);

}  // namespace qla
