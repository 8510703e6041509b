// ballot_audit_device.h — the device path of the log audit as host code calls
// it (ballot_audit.cpp): the passes over an uploaded log that fill
// qb::AuditFacts.  qp_ballot_log_audit runs them on buffers of its own,
// qp_ballot_box_restore (ballot.cpp) on the new box's log and table, which it
// then keeps.
#pragma once
#include <stdint.h>
#include <string>
#include "acc_tree.h"
#include "ballot_audit.h"
#include "ballot_kernels.h"
#include "ctx.h"

namespace qba {

// The passes over log [0, n), 1 <= n <= 2^31, which the caller enqueued for
// upload into d on c's stream, with d's table all-empty and S >= 2 n slots:
// the screen (then a synchronise: on a non-canonical log nothing is hashed and
// *canonical is false), the whole-log insert, the count rule and the counts,
// and, with `tree` (an AccTree without a tree, which this call allocates for n
// leaves), the log's leaves and the levels above them.  One more synchronise;
// afterwards d's table is the table of that log and `tree` holds n leaves.
// QP_ERR_HIP / QP_ERR_OOM: a HIP step failed; QP_ERR_STATE: the defensive error
// word was set.  The caller has set the device.
int audit_facts_device(qp_ctx *c, AccErr e, const qpk::BallotDev &d, uint64_t n, AccTree *tree, qb::AuditFacts &f,
                       bool *canonical);

// the reason of a call that has no box to carry it: qp_ballot_box_last_error(NULL)'s text on this
// thread, and c's err when there is a context (ballot.cpp)
void set_boxless_error(qp_ctx *c, const std::string &why);

}  // namespace qba
