// ledger_rounds.cpp — payout rounds (qpgpu.h): the device path both forms share
// and qp_ledger_log_payouts_between, the form that needs no ledger.  The rule
// and the host path are ledger_rounds.h's; qp_ledger_payouts_between is with the
// ledger's other entry points in ledger.cpp.
#include "../../include/qpgpu.h"
#include <string.h>
#include <algorithm>
#include <new>
#include <string>
#include "acc_tree.h"
#include "ledger_audit_device.h"
#include "ledger_kernels.h"
#include "ledger_rounds.h"

// Launch order on the one stream, every buffer but the log the call's own: the credit of the range
// into the scratch account table and its sums; the owners' count per block, the scan, the owners'
// write (log order = first_seq order, no sort); a synchronise for the row count.  A sum or a slot word
// is read only in launches after the one that writes it.
int qla::round_credit_device(qp_ctx *c, std::string &err, const uint64_t *accounts_at_m0, const uint32_t *amounts_at_m0,
                             const uint8_t *flags_at_m0, uint64_t k, RoundCredit &r) {
  AccErr e{err};
  hipStream_t s = c->stream;
  const uint64_t S = ql::table_slots(k);
  const uint32_t nb = qpk::ledger_blocks(k);
  QP_HIP_TRY(&e, hipSetDevice(c->device));
  QP_HIP_TRY(&e, r.astay.alloc((size_t)((k + 1) / 2)));
  QP_HIP_TRY(&e, r.aslot.alloc((size_t)(S / 2)));
  QP_HIP_TRY(&e, r.sum.alloc((size_t)(S * 4)));
  QP_HIP_TRY(&e, r.d_err.alloc(1));
  QP_HIP_TRY(&e, r.d_blk.alloc(((size_t)nb + 2) / 2));
  QP_HIP_TRY(&e, r.d_payee.alloc((size_t)((k + 1) / 2)));
  r.v = qpk::LedgerDev{nullptr,
                       nullptr,
                       const_cast<uint32_t *>(amounts_at_m0),
                       const_cast<uint64_t *>(accounts_at_m0),
                       const_cast<uint8_t *>(flags_at_m0),
                       r.astay.as<uint32_t>(),
                       nullptr,
                       r.aslot.as<uint32_t>(),
                       r.sum.as<unsigned long long>(),
                       S - 1};
  const qpk::LedgerDev &v = r.v;
  uint32_t *blk = r.d_blk.as<uint32_t>(), *payee = r.d_payee.as<uint32_t>(), rows = 0, bad = 0;
  QP_HIP_TRY(&e, hipMemsetAsync(r.aslot.p, 0xFF, S * 4, s));
  QP_HIP_TRY(&e, hipMemsetAsync(r.sum.p, 0, S * 32, s));
  QP_HIP_TRY(&e, hipMemsetAsync(r.d_err.p, 0, 8, s));
  qpk::ledger_round_credit(v, (uint32_t)k, r.d_err.as<uint32_t>(), s);
  QP_HIP_TRY(&e, hipGetLastError());
  qpk::ledger_payee_count(v, (uint32_t)k, blk, s);
  QP_HIP_TRY(&e, hipGetLastError());
  qpk::ledger_scan(blk, nb, blk + nb, s);
  QP_HIP_TRY(&e, hipGetLastError());
  qpk::ledger_payee_write(v, (uint32_t)k, blk, payee, s);
  QP_HIP_TRY(&e, hipGetLastError());
  QP_HIP_TRY(&e, hipMemcpyAsync(&rows, blk + nb, 4, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(&e, hipMemcpyAsync(&bad, r.d_err.p, 4, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(&e, hipStreamSynchronize(s));
  if (bad || rows > k) {
    err = std::string(bad ? "the round's account table's probe found no slot"
                          : "the round's compaction counted more accounts than the range has entries") +
          " (an internal invariant broke)";
    return QP_ERR_HIP;
  }
  r.rows = rows;
  return QP_OK;
}

// The round's rows after the credit: one gather of the first min(cap, rows) rows.
int qla::rounds_device(qp_ctx *c, std::string &err, const uint64_t *accounts_at_m0, const uint32_t *amounts_at_m0,
                       const uint8_t *flags_at_m0, uint64_t k, uint64_t m0, uint64_t cap, uint64_t *accounts,
                       uint64_t *sums, uint64_t *first_seq, uint64_t *count) {
  AccErr e{err};
  hipStream_t s = c->stream;
  RoundCredit r;
  DevBuf o_acc, o_sum, o_seq;
  if (int rc = round_credit_device(c, err, accounts_at_m0, amounts_at_m0, flags_at_m0, k, r)) return rc;
  const qpk::LedgerDev &v = r.v;
  const uint32_t *payee = r.payee(), rows = r.rows;
  const uint32_t stored = (uint32_t)std::min<uint64_t>(cap, rows);
  if (stored) {
    QP_HIP_TRY(&e, o_acc.alloc((size_t)stored * 4));
    QP_HIP_TRY(&e, o_sum.alloc((size_t)stored * 4));
    QP_HIP_TRY(&e, o_seq.alloc(stored));
    qpk::ledger_payouts(v, payee, stored, o_acc.p, o_sum.as<unsigned long long>(), o_seq.p, s);
    QP_HIP_TRY(&e, hipGetLastError());
    QP_HIP_TRY(&e, hipMemcpyAsync(accounts, o_acc.p, (size_t)stored * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipMemcpyAsync(sums, o_sum.p, (size_t)stored * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipMemcpyAsync(first_seq, o_seq.p, (size_t)stored * 8, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < stored; i++) first_seq[i] += m0;  // the view counts from m0
  }
  *count = rows;
  return QP_OK;
}

namespace {
int log_rounds_device(qp_ctx *c, const uint64_t *accounts_log, const uint32_t *amounts, const uint8_t *flags, uint64_t m0,
                      uint64_t m1, uint64_t cap, uint64_t *accounts, uint64_t *sums, uint64_t *first_seq,
                      uint64_t *count) {
  hipStream_t s = c->stream;
  const uint64_t k = m1 - m0;
  DevBuf acc, amt, fl;
  QP_HIP_TRY(c, hipSetDevice(c->device));
  QP_HIP_TRY(c, acc.alloc((size_t)k * 4));
  QP_HIP_TRY(c, amt.alloc((size_t)k * 2));
  QP_HIP_TRY(c, fl.alloc((size_t)((k + 7) / 8)));
  QP_HIP_TRY(c, hipMemcpyAsync(acc.p, accounts_log + m0 * 4, (size_t)k * 32, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipMemcpyAsync(amt.p, amounts + m0 * 4, (size_t)k * 16, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipMemcpyAsync(fl.p, flags + m0, (size_t)k, hipMemcpyHostToDevice, s));
  return qla::rounds_device(c, c->err, acc.p, amt.as<uint32_t>(), fl.as<uint8_t>(), k, m0, cap, accounts, sums,
                            first_seq, count);
}
}  // namespace

extern "C" int qp_ledger_log_payouts_between(qp_ctx *c, const uint64_t *accounts_log, const uint32_t *amounts,
                                             const uint8_t *flags, uint64_t n, uint64_t m0, uint64_t m1, uint64_t cap,
                                             uint64_t *accounts, uint64_t *sums, uint64_t *first_seq, uint64_t *count) {
  auto refuse = [c](int rc, const std::string &why) {
    qla::set_ledgerless_error(c, "qp_ledger_log_payouts_between: " + why);
    return rc;
  };
  if (!accounts_log || !amounts || !flags) return refuse(QP_ERR_ARG, "null log buffer");
  if (!n || n > ql::MAX_CAPACITY)
    return refuse(QP_ERR_ARG, "a log of " + std::to_string(n) + " entries: a published log has 1 to 2^31");
  std::string why = ql::round_refusal(n, m0, m1, cap, accounts, sums, first_seq, count);
  if (why.empty()) why = ql::round_log_refusal(accounts_log, flags, m0, m1);
  if (!why.empty()) return refuse(QP_ERR_ARG, why);
  if (m0 == m1) {
    *count = 0;
    return QP_OK;
  }
  try {
    if (!c) {
      ql::RoundRows rows;
      ql::round_payouts_host(accounts_log, amounts, flags, m0, m1, rows);
      ql::round_store(rows, cap, accounts, sums, first_seq, count);
      return QP_OK;
    }
    const int rc = log_rounds_device(c, accounts_log, amounts, flags, m0, m1, cap, accounts, sums, first_seq, count);
    return rc ? refuse(rc, c->err) : QP_OK;
  } catch (const std::bad_alloc &) {
    return refuse(QP_ERR_OOM, "out of host memory");
  }
}
