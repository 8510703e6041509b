// claims.cpp — the payout claims entry points (qpgpu.h) that need no ledger:
// the claims commitment of a range of a published log on either path (a
// ClaimsCommit of the call's own, claims_commit.h), the checker of a claim
// (claims.h; host only) and the stage times of the last device build.  The
// ledger's calls (qp_ledger_commit_claims, qp_ledger_claims) are in ledger.cpp.
#include "../../include/qpgpu.h"
#include <string.h>
#include <new>
#include <string>
#include <vector>
#include "claims.h"
#include "claims_commit.h"
#include "ctx.h"
#include "ledger_audit_device.h"
#include "ledger_rounds.h"

namespace {
int log_claims_device(qp_ctx *c, ClaimsCommit &cc, const uint64_t *accounts_log, const uint32_t *amounts,
                      const uint8_t *flags, uint64_t m0, uint64_t m1, uint64_t *order_out) {
  hipStream_t s = c->stream;
  const uint64_t k = m1 - m0;
  DevBuf acc, amt, fl;  // the range alone, alive until the commitment's last synchronise
  QP_HIP_TRY(c, hipSetDevice(c->device));
  if (k) {
    QP_HIP_TRY(c, acc.alloc((size_t)k * 4));
    QP_HIP_TRY(c, amt.alloc((size_t)k * 2));
    QP_HIP_TRY(c, fl.alloc((size_t)((k + 7) / 8)));
    QP_HIP_TRY(c, hipMemcpyAsync(acc.p, accounts_log + m0 * 4, (size_t)k * 32, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(c, hipMemcpyAsync(amt.p, amounts + m0 * 4, (size_t)k * 16, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(c, hipMemcpyAsync(fl.p, flags + m0, (size_t)k, hipMemcpyHostToDevice, s));
  }
  if (int rc = cc.commit_device(c, c->err, acc.p, amt.as<uint32_t>(), fl.as<uint8_t>(), m0, m1)) return rc;
  return order_out ? cc.order_device(c, c->err, order_out) : QP_OK;
}
}  // namespace

extern "C" {

uint32_t qp_ledger_claims_times(double *ms, uint32_t cap) {
  const std::vector<double> &t = claims_commit_last_times();
  if (!ms || cap < t.size()) return 0;
  for (size_t i = 0; i < t.size(); i++) ms[i] = t[i];
  return (uint32_t)t.size();
}

int qp_ledger_log_claims_root(qp_ctx *c, const uint64_t *accounts_log, const uint32_t *amounts, const uint8_t *flags,
                              uint64_t n, uint64_t m0, uint64_t m1, uint64_t root_out[4], uint64_t *count_out,
                              uint32_t total_out[5], uint64_t *order_out) {
  auto refuse = [c](int rc, const std::string &why) {
    qla::set_ledgerless_error(c, "qp_ledger_log_claims_root: " + why);
    return rc;
  };
  if (!accounts_log || !amounts || !flags) return refuse(QP_ERR_ARG, "null log buffer");
  if (!n || n > ql::MAX_CAPACITY)
    return refuse(QP_ERR_ARG, "a log of " + std::to_string(n) + " entries: a published log has 1 to 2^31");
  uint64_t count = 0;
  std::string why = ql::round_refusal(n, m0, m1, 0, nullptr, nullptr, nullptr, &count);
  if (why.empty()) why = ql::round_log_refusal(accounts_log, flags, m0, m1);
  if (!why.empty()) return refuse(QP_ERR_ARG, why);
  try {
    ClaimsCommit cc;
    if (c) {
      if (int rc = log_claims_device(c, cc, accounts_log, amounts, flags, m0, m1, order_out)) return refuse(rc, c->err);
    } else {
      cc.commit_host(accounts_log, amounts, flags, m0, m1);
      if (order_out)
        for (uint64_t j = 0; j < cc.A; j++) order_out[j] = cc.host.first_seq[j];
    }
    cc.triple(root_out, count_out, total_out);
    return QP_OK;
  } catch (const std::bad_alloc &) {
    return refuse(QP_ERR_OOM, "out of host memory");
  }
}

int qp_ledger_claim_check(const uint64_t root[4], uint64_t count, const uint64_t x[4], uint32_t found, uint64_t pos,
                          const uint64_t lo_account[4], const uint32_t lo_total[5], uint64_t lo_first_seq,
                          const uint64_t *lo_siblings, uint32_t lo_bits, uint32_t lo_depth, const uint64_t hi_account[4],
                          const uint32_t hi_total[5], uint64_t hi_first_seq, const uint64_t *hi_siblings,
                          uint32_t hi_bits, uint32_t hi_depth) {
  if (!root || !x || !lo_account || !lo_total || !lo_siblings || !hi_account || !hi_total || !hi_siblings)
    return QP_RECEIPT_NULL;
  return qcl::check(root, count, x, found, pos,
                    qcl::Slot{lo_account, lo_total, lo_first_seq, lo_siblings, lo_bits, lo_depth},
                    qcl::Slot{hi_account, hi_total, hi_first_seq, hi_siblings, hi_bits, hi_depth});
}

}  // extern "C"
