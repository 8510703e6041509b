// ballot_audit_device.h — the device path of the log audit as host code calls
// it (ballot_audit.cpp): the passes over an uploaded log that fill
// qb::AuditFacts.  qp_ballot_log_audit runs them on buffers of its own,
// qp_ballot_box_restore (ballot.cpp) on the new box's log and table, which it
// then keeps.  DeviceTables is the device half of a box for one capacity: the
// box holds one, a reserve builds the next beside it, and an audit one for its call.
#pragma once
#include <stdint.h>
#include <string>
#include "acc_tree.h"
#include "ballot_audit.h"
#include "ballot_kernels.h"
#include "ballot_table.h"
#include "ctx.h"

namespace qba {

// the device half of a box for one capacity: the log, the table
struct DeviceTables {
  DevBuf nul, num, flags, slot;
  uint64_t mask = 0;
  qpk::BallotDev dev() const {
    return qpk::BallotDev{nul.p, num.p, flags.as<uint8_t>(), slot.as<uint32_t>(), mask};
  }
};

// t for `capacity` entries, its table all-empty (a memset enqueued on s)
inline int alloc_tables(AccErr e, hipStream_t s, uint64_t capacity, DeviceTables &t) {
  const uint64_t S = qb::table_slots(capacity);
  QP_HIP_TRY(&e, t.nul.alloc(capacity * 4));
  QP_HIP_TRY(&e, t.num.alloc(capacity));
  QP_HIP_TRY(&e, t.flags.alloc((capacity + 7) / 8));
  QP_HIP_TRY(&e, t.slot.alloc(S / 2));
  t.mask = S - 1;
  QP_HIP_TRY(&e, hipMemsetAsync(t.slot.p, 0xFF, S * 4, s));
  return QP_OK;
}

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
