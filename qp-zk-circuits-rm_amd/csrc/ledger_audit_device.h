// ledger_audit_device.h — what ledger_audit.cpp (qp_ledger_log_audit) shares
// with ledger.cpp beside the headers of the kernels and of the rules.
#pragma once
#include <string>
#include "ctx.h"

namespace qla {

// the reason of a call that has no ledger to carry it: qp_ledger_last_error(NULL)'s text on this
// thread, and c's err when there is a context (ledger.cpp)
void set_ledgerless_error(qp_ctx *c, const std::string &why);

}  // namespace qla
